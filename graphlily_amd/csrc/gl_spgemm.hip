// SpGEMM (gl_spgemm_symbolic / gl_spgemm_numeric, graphlily_hip_spgemm.h): C = A (+).(x) B with a sparse result and an optional
// structural mask, over the plain CSR copies that GL_PLAN_BOOLEAN plans keep, on square, whole-matrix plans whose rows are strictly
// ascending sets (gl_rows.h: kRowsSets).  The values travel apart from the plans, an f32 per entry of the row copy.
//
// ROW-WISE (Gustavson): one agent owns row i of C.  For every k in A(i) it streams B(k) -- a group of `group` lanes per k, the
// groups of the agent side by side, so that short rows of B fill a wavefront -- and inserts every column the mask admits into a
// table of (key, accumulator) slots: the key is claimed by compare-and-swap on the empty key 0xffffffff at (107 column) mod T,
// linear probing behind it; the accumulator is a 64-bit LDS word that STARTS AS ZERO BITS under every semiring:
//   (+,x)    an f64: the product of two f32 is exact in f64, the adds are f64 atomics, one rounding to f32 at emission
//   (min,+)  the COMPLEMENT of gl_msf's monotone f32 -> uint32 key of a + b (f32), under an integer atomic max: bit-exact
// A row's table is min(Tmax, the power of two >= 2 count) slots of the path's room, so a short row clears and sorts little.
//
// THREE PATHS, a row's by its count -- symbolic: its products, an upper bound of |C(i)| (one streaming pass, cached in plan a with
// the bins, for the last partner b); numeric: |C(i)| itself from d_c_indptr (binned per call: the tables are tight, and a row
// whose bound was huge but whose result is short is back in LDS) --, the bin lists compacted in row order by gl_compact.h:
//   wavefront   count <= spgemm_wave_slots (512)   four wavefronts per workgroup, each with its own table; wavefront fences only
//   workgroup   count <= spgemm_lds_slots (8192)   eight wavefronts share a table in dynamic LDS (96 KiB of keys and accumulators,
//                                                  above 64 KiB by hipFuncSetAttribute) and the mask row, staged up to 4096 entries
//   slab        above                              a dense accumulator over the n columns -- a bitmap and a 64-bit word per column
//                                                  -- in one of a fixed number of global slabs, one per workgroup, cleaned by the
//                                                  row that used it; emission from the bitmap is already in column order
// spgemm_wave=0 closes the first path, spgemm_lds=0 the first two.  Every default is a starting value (EXPERIMENTS.md Round 32).
// The hash paths compact the occupied slots in place, then sort (key, accumulator) in LDS: up to 64 entries by counting the
// smaller keys, above by a bitonic network over the next power of two.  Symbolic runs the same paths with keys only, counts the
// claims, and one exclusive scan (one workgroup, 64-bit carry) turns the counts into d_c_indptr.
// No spin-waits, no hand-offs between workgroups, no f32 atomic.  A probe gives up after T slots and emission writes at most the
// d_c_indptr's room, so a d_c_indptr that is not the symbolic call's loses entries but writes nothing out of bounds.
#include "gl_compact.h"
#include "gl_rows.h"
#include "graphlily_hip_spgemm.h"

#include <algorithm>

namespace gl {

constexpr uint32_t kSpgemmEmpty = 0xffffffffu;
constexpr uint32_t kSpgemmWaveMax = 512, kSpgemmLdsMax = 8192, kSpgemmMinSlots = 64, kSpgemmMaskStage = 4096, kSpgemmRankMax = 64;
constexpr uint32_t kSpgemmWaveThreads = 256, kSpgemmThreads = 512;
constexpr uint32_t kSpgemmLdsOptIn = 64u * 1024u;   // what a launch gets without asking
// what a kernel computes: the row counts from keys alone, C's columns alone ((||,&&): no value is read), or values too
enum : int { kSpgemmSymbolic = 0, kSpgemmPattern = 1, kSpgemmMulAdd = 2, kSpgemmAddMin = 3 };

struct SpgemmArgs {
    const uint32_t *a_ptr, *a_idx, *b_ptr, *b_idx, *m_ptr, *m_idx;
    const float *a_val, *b_val;
    const gl_idx_val *items;               // gl_compact.h's list: items[0].index rows, their numbers in items[1 ..].index
    const uint32_t *bound;                 // symbolic: the rows' products
    const uint32_t *c_ptr;                 // numeric: d_c_indptr
    uint32_t *counts;                      // symbolic: |C(i)| per row (d_c_indptr before the scan)
    uint32_t *c_idx;
    float *c_val;
    uint32_t *slab_bits;                   // slab path: slab_words words of bitmap per workgroup ...
    unsigned long long *slab_val;          // ... and n accumulators
    uint32_t a_base, b_base, m_base, n;
    uint32_t tmax;                         // slots the launch has room for per agent, a power of two
    uint32_t group;                        // lanes that stream one row of B, a power of two <= 64
    uint32_t mask_mode;                    // 0 none, 1 stored entries admit, 2 stored entries refuse
    uint32_t slab_words;
};

// ---------------------------------------------------------------------------------------------------------------- the agents
// a wavefront (fences) or a workgroup (barriers) of `size` threads
template <bool WG>
struct SpgemmTeam {
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

// exclusive prefix of v over the team, in thread order, the sum in *total; wsum: 17 words of the workgroup's LDS
template <bool WG, typename T>
__device__ __forceinline__ T spgemm_scan(const SpgemmTeam<WG> &t, T v, unsigned long long *wsum, T *total) {
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

__device__ __forceinline__ uint32_t spgemm_key(float w) {   // gl_msf.hip: the monotone map of f32 to uint32
    const uint32_t b = __float_as_uint(w);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float spgemm_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// one product into an accumulator that started as zero bits (LDS or a slab: the pointer is generic)
template <int MODE>
__device__ __forceinline__ void spgemm_accumulate(unsigned long long *acc, float av, float bv) {
    if (MODE == kSpgemmMulAdd) atomicAdd(reinterpret_cast<double *>(acc), (double)av * (double)bv);
    if (MODE == kSpgemmAddMin) atomicMax(reinterpret_cast<uint32_t *>(acc), ~spgemm_key(av + bv));
}
template <int MODE>
__device__ __forceinline__ float spgemm_value(unsigned long long acc) {
    if (MODE == kSpgemmMulAdd) return (float)__longlong_as_double((long long)acc);
    if (MODE == kSpgemmAddMin) return spgemm_unkey(~(uint32_t)acc);
    return 1.0f;
}

// does the mask admit column c of this row?  mrow: the mask's row, ascending, mlen entries (LDS or global)
__device__ __forceinline__ bool spgemm_admits(uint32_t mode, const uint32_t *mrow, uint32_t mlen, uint32_t c) {
    if (mode == 0u) return true;
    const bool stored = mlen != 0u && mrow[rows_lower_bound(mrow, mlen, c)] == c;
    return stored != (mode == 2u);
}

// THE STREAM of one row of C: visit(column, a's value, b's value) for every product the mask admits
template <int MODE, typename Visit>
__device__ __forceinline__ void spgemm_stream(const SpgemmArgs &g, uint32_t i, uint32_t tid, uint32_t size, const uint32_t *mrow,
                                              uint32_t mlen, Visit &&visit) {
    const uint32_t ab = g.a_ptr[i] - g.a_base, da = g.a_ptr[i + 1u] - g.a_ptr[i];
    const uint32_t grp = tid / g.group, gl = tid & (g.group - 1u), groups = size / g.group;
    for (uint32_t ai = grp; ai < da; ai += groups) {
        const uint32_t k = g.a_idx[ab + ai];                                 // < n: established by rows_require
        const float av = MODE >= kSpgemmMulAdd ? g.a_val[ab + ai] : 0.0f;
        const uint32_t bb = g.b_ptr[k] - g.b_base, db = g.b_ptr[k + 1u] - g.b_ptr[k];
        for (uint32_t j = gl; j < db; j += g.group) {
            const uint32_t c = g.b_idx[bb + j];
            if (!spgemm_admits(g.mask_mode, mrow, mlen, c)) continue;
            visit(c, av, MODE >= kSpgemmMulAdd ? g.b_val[bb + j] : 0.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- the two hash paths
// LDS of a launch, in 64-bit words first: [accumulators: agents x tmax] [17 words of scan room] then 32-bit words: [keys: agents
// x tmax] [one count word] [the staged mask row: kSpgemmMaskStage, workgroup path with a mask only]
template <int MODE, bool WG>
__global__ __launch_bounds__(WG ? kSpgemmThreads : kSpgemmWaveThreads) void spgemm_hash_kernel(SpgemmArgs g) {
    extern __shared__ unsigned long long spgemm_lds[];
    const uint32_t agents = WG ? 1u : blockDim.x >> 6, agent = WG ? 0u : threadIdx.x >> 6;
    SpgemmTeam<WG> t;
    t.tid = WG ? threadIdx.x : threadIdx.x & 63u;
    t.size = WG ? blockDim.x : 64u;
    unsigned long long *vals = spgemm_lds + (MODE >= kSpgemmMulAdd ? agent * g.tmax : 0u);
    unsigned long long *wsum = spgemm_lds + (MODE >= kSpgemmMulAdd ? agents * g.tmax : 0u);
    uint32_t *words = reinterpret_cast<uint32_t *>(wsum + 17);
    uint32_t *keys = words + agent * g.tmax;
    uint32_t *claims = words + agents * g.tmax;
    uint32_t *mstage = claims + 1;
    const uint32_t nitems = g.items[0].index;
    for (uint32_t it = WG ? blockIdx.x : blockIdx.x * agents + agent; it < nitems; it += gridDim.x * agents) {
        const uint32_t i = g.items[1u + it].index;
        const uint32_t out = MODE ? g.c_ptr[i] : 0u;
        const uint32_t count = MODE ? g.c_ptr[i + 1u] - out : g.bound[i];     // 1 .. tmax: the bin's rule
        uint32_t T = kSpgemmMinSlots;
        while (T < g.tmax && T < 2u * count) T <<= 1;
        const uint32_t *mrow = nullptr;
        uint32_t mlen = 0;
        if (g.mask_mode) {
            mrow = g.m_idx + (g.m_ptr[i] - g.m_base);
            mlen = g.m_ptr[i + 1u] - g.m_ptr[i];
        }
        t.sync();                                                            // the last row's table has been read
        for (uint32_t s = t.tid; s < T; s += t.size) {
            keys[s] = kSpgemmEmpty;
            if (MODE >= kSpgemmMulAdd) vals[s] = 0ull;
        }
        if (WG) {
            if (t.tid == 0u) *claims = 0u;
            if (g.mask_mode && mlen <= kSpgemmMaskStage) {
                for (uint32_t s = t.tid; s < mlen; s += t.size) mstage[s] = mrow[s];
                mrow = mstage;
            }
        }
        t.sync();
        uint32_t claimed = 0;
        spgemm_stream<MODE>(g, i, t.tid, t.size, mrow, mlen, [&](uint32_t c, float av, float bv) {
            uint32_t h = (c * 107u) & (T - 1u);
            for (uint32_t probe = 0; probe < T; probe++) {
                const uint32_t old = atomicCAS(keys + h, kSpgemmEmpty, c);
                if (old == kSpgemmEmpty || old == c) {
                    spgemm_accumulate<MODE>(vals + h, av, bv);
                    claimed += old == kSpgemmEmpty ? 1u : 0u;
                    break;
                }
                h = (h + 1u) & (T - 1u);
            }
        });
        if (MODE == kSpgemmSymbolic) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) claimed += __shfl_xor(claimed, off);
            if (WG) {
                if ((t.tid & 63u) == 0u && claimed) atomicAdd(claims, claimed);
                __syncthreads();
                claimed = *claims;
            }
            if (t.tid == 0u) g.counts[i] = claimed;
            continue;
        }
        t.sync();
        // compact the occupied slots to the front, in place: a piece is read by everyone before anyone writes, and what is
        // written lies in front of the pieces still to be read
        uint32_t have = 0;
        for (uint32_t s0 = 0; s0 < T; s0 += t.size) {
            const uint32_t s = s0 + t.tid;
            const uint32_t key = s < T ? keys[s] : kSpgemmEmpty;
            const unsigned long long val = MODE >= kSpgemmMulAdd && s < T ? vals[s] : 0ull;
            uint32_t total;
            const uint32_t rank = spgemm_scan<WG, uint32_t>(t, key != kSpgemmEmpty ? 1u : 0u, wsum, &total);
            t.sync();
            if (key != kSpgemmEmpty) {
                keys[have + rank] = key;
                if (MODE >= kSpgemmMulAdd) vals[have + rank] = val;
            }
            have += total;
            t.sync();
        }
        const uint32_t cc = min(have, count);                                // (have == count for the symbolic call's d_c_indptr)
        if (cc <= kSpgemmRankMax) {
            // a short row: an entry's place is the number of smaller keys
            if (t.tid < cc) {
                const uint32_t key = keys[t.tid];
                uint32_t r = 0;
                for (uint32_t j = 0; j < cc; j++) r += keys[j] < key ? 1u : 0u;
                g.c_idx[out + r] = key;
                if (g.c_val) g.c_val[out + r] = spgemm_value<MODE>(MODE >= kSpgemmMulAdd ? vals[t.tid] : 0ull);
            }
            continue;
        }
        uint32_t P = kSpgemmMinSlots;
        while (P < cc) P <<= 1;                                              // <= T: cc <= T and T is a power of two
        for (uint32_t s = cc + t.tid; s < P; s += t.size) keys[s] = kSpgemmEmpty;
        t.sync();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t p = t.tid; p < (P >> 1); p += t.size) {
                    const uint32_t lo = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), hi = lo | j;
                    const uint32_t kl = keys[lo], kh = keys[hi];
                    if ((kl > kh) == ((lo & k) == 0u)) {
                        keys[lo] = kh;
                        keys[hi] = kl;
                        if (MODE >= kSpgemmMulAdd) {
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
            if (g.c_val) g.c_val[out + s] = spgemm_value<MODE>(MODE >= kSpgemmMulAdd ? vals[s] : 0ull);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- the slab path
// a word that atomics of other wavefronts wrote, which the vector cache does not see (gl_clique.hip: clique_word)
template <typename T>
__device__ __forceinline__ T spgemm_slab_load(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void spgemm_slab_clear(T *p) {
    __hip_atomic_store(p, (T)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int MODE>
__global__ __launch_bounds__(kSpgemmThreads) void spgemm_slab_kernel(SpgemmArgs g) {
    __shared__ unsigned long long wsum[17];
    SpgemmTeam<true> t;
    t.tid = threadIdx.x;
    t.size = blockDim.x;
    uint32_t *bits = g.slab_bits + (size_t)blockIdx.x * g.slab_words;        // all zero between rows
    unsigned long long *vals = g.slab_val + (size_t)blockIdx.x * g.n;
    const uint32_t nitems = g.items[0].index;
    for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        const uint32_t i = g.items[1u + it].index;
        const uint32_t out = MODE ? g.c_ptr[i] : 0u, room = MODE ? g.c_ptr[i + 1u] - out : 0u;
        const uint32_t *mrow = nullptr;
        uint32_t mlen = 0;
        if (g.mask_mode) {
            mrow = g.m_idx + (g.m_ptr[i] - g.m_base);
            mlen = g.m_ptr[i + 1u] - g.m_ptr[i];
        }
        spgemm_stream<MODE>(g, i, t.tid, t.size, mrow, mlen, [&](uint32_t c, float av, float bv) {   // c < n: rows_require
            atomicOr(bits + (c >> 5), 1u << (c & 31u));
            spgemm_accumulate<MODE>(vals + c, av, bv);
        });
        __threadfence();
        __syncthreads();
        // emit from the bitmap, which is in column order, and leave the slab as it was found
        uint32_t running = 0;
        for (uint32_t w0 = 0; w0 < g.slab_words; w0 += t.size) {
            const uint32_t wi = w0 + t.tid;
            const uint32_t w = wi < g.slab_words ? spgemm_slab_load(bits + wi) : 0u;
            uint32_t total;
            uint32_t pos = running + spgemm_scan<true, uint32_t>(t, (uint32_t)__popc(w), wsum, &total);
            if (w != 0u) {
                for (uint32_t r = w; MODE != kSpgemmSymbolic && r; r &= r - 1u, pos++) {
                    const uint32_t c = wi * 32u + (uint32_t)__ffs((int)r) - 1u;
                    unsigned long long acc = 0ull;
                    if (MODE >= kSpgemmMulAdd) {
                        acc = spgemm_slab_load(vals + c);
                        spgemm_slab_clear(vals + c);
                    }
                    if (pos < room) {
                        g.c_idx[out + pos] = c;
                        if (g.c_val) g.c_val[out + pos] = spgemm_value<MODE>(acc);
                    }
                }
                spgemm_slab_clear(bits + wi);
            }
            running += total;
        }
        if (MODE == kSpgemmSymbolic && t.tid == 0u) g.counts[i] = running;
        __threadfence();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------ the streaming passes
// bound[i] = the products of row i (saturating), *total += their sum
__global__ __launch_bounds__(256) void spgemm_bound_kernel(const uint32_t *a_ptr, const uint32_t *a_idx, uint32_t a_base, const uint32_t *b_ptr,
                                                           uint32_t n, uint32_t *bound, unsigned long long *total) {
    unsigned long long mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned long long sum = 0;
        for (uint32_t e = a_ptr[i] - a_base, end = a_ptr[i + 1u] - a_base; e < end; e++) {
            const uint32_t k = a_idx[e];
            sum += b_ptr[k + 1u] - b_ptr[k];
        }
        bound[i] = (uint32_t)min(sum, 0xffffffffull);
        mine += sum;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(total, mine);
}

__global__ __launch_bounds__(256) void spgemm_zero_kernel(uint32_t *x, uint32_t words, unsigned long long *also) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) x[i] = 0u;
    if (also && blockIdx.x == 0u && threadIdx.x == 0u) *also = 0ull;
}

// x[0 .. n) counts -> x[0 .. n] exclusive offsets (32 bits each), the 64-bit sum in *total: one workgroup
__global__ __launch_bounds__(1024) void spgemm_offsets_kernel(uint32_t *x, uint32_t n, unsigned long long *total) {
    __shared__ unsigned long long wsum[17];
    SpgemmTeam<true> t;
    t.tid = threadIdx.x;
    t.size = blockDim.x;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < n; base += t.size) {
        const uint32_t i = base + t.tid;
        unsigned long long sum;
        const unsigned long long before = spgemm_scan<true, unsigned long long>(t, i < n ? x[i] : 0u, wsum, &sum);
        if (i < n) x[i] = (uint32_t)(carry + before);
        carry += sum;
    }
    if (t.tid == 0u) {
        x[n] = (uint32_t)carry;
        *total = carry;
    }
}

// gl_compact.h's source: the rows whose count -- v[i], or the length of row i of ptr -- lies in (lo, hi]
struct SpgemmBinSrc {
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
// plan a's scratch: 256 bytes of control words (64-bit: 0 the products, 1 nnz(C)), n bounds, gl_compact.h's counts, six lists
struct SpgemmScratch {
    unsigned long long *ctl;
    uint32_t *bound, *compact;
    gl_idx_val *list[6];               // 0 .. 2 symbolic (cached), 3 .. 5 numeric (per call): wavefront, workgroup, slab
};
static size_t spgemm_scratch_map(unsigned char *base, uint32_t n, SpgemmScratch *m) {
    size_t at = 256;
    m->ctl = reinterpret_cast<unsigned long long *>(base);
    m->bound = reinterpret_cast<uint32_t *>(base + at);
    at += (((size_t)n + 1u) & ~(size_t)1u) * 4u;
    for (auto &l : m->list) {
        l = reinterpret_cast<gl_idx_val *>(base + at);
        at += ((size_t)n + 1u) * 8u;
    }
    m->compact = reinterpret_cast<uint32_t *>(base + at);
    at += ((size_t)cdiv(std::max(n, 1u), kCompactChunk) + 2u) * 4u;
    return at;
}

static uint32_t spgemm_pow2_floor(long v, uint32_t lo, uint32_t hi) {
    uint32_t p = lo;
    while (p < hi && (long)p * 2 <= v) p <<= 1;
    return p;
}

// three lists by the cuts of plan a: counts in (0, wave], (wave, lds], above
static int spgemm_bin(gl_spmv_plan a, const SpgemmScratch &m, int first, const uint32_t *v, const uint32_t *ptr) {
    const uint32_t cut[4] = {0u, a->spgemm_wave_slots, a->spgemm_lds_slots, 0xffffffffu};
    for (int b = 0; b < 3; b++) {
        const SpgemmBinSrc src{v, ptr, a->num_rows, cut[b], cut[b + 1]};
        const int rc = run_compaction(src, a->num_rows, m.compact, m.list[first + b], 0.0f, ctx().stream);
        if (rc != GL_OK) return rc;
    }
    return GL_OK;
}

static int spgemm_list_sizes(const SpgemmScratch &m, int first, uint32_t *sizes) {
    for (int b = 0; b < 3; b++) GL_HIP(hipMemcpy(sizes + b, &m.list[first + b][0].index, 4, hipMemcpyDeviceToHost));
    return GL_OK;
}

// what plan a keeps for its partner b, on first use (one synchronisation): knobs, bounds, symbolic bins, slabs
static int spgemm_prepare(gl_spmv_plan a, gl_spmv_plan b, const char *who) {
    if (a->d_spgemm_scratch && a->spgemm_partner == b && a->spgemm_partner_uid == b->uid) return GL_OK;
    hipStream_t s = ctx().stream;
    const uint32_t n = a->num_rows;
    SpgemmScratch m;
    const size_t bytes = spgemm_scratch_map(nullptr, n, &m);
    const bool fresh = a->d_spgemm_scratch == nullptr;
    int rc = plan_scratch(a->d_spgemm_scratch, bytes, who, "bounds and bin lists");
    if (rc != GL_OK) return rc;
    spgemm_scratch_map(a->d_spgemm_scratch, n, &m);
    a->spgemm_partner = nullptr;
    // A/B knobs (GRAPHLILY_DEBUG, read by the plan's first call with a partner): spgemm_wave / spgemm_lds = 0 close the wavefront
    // path / both hash paths, spgemm_wave_slots / spgemm_lds_slots = their tables (powers of two from 64), spgemm_group = lanes
    // per row of B (0: the power of two at or above B's mean row, 4 .. 64), spgemm_scratch_mb = room for the slabs.  ALL GUESSES.
    const bool use_lds = debug_knob("spgemm_lds", 1) != 0, use_wave = use_lds && debug_knob("spgemm_wave", 1) != 0;
    const uint32_t lds_slots = spgemm_pow2_floor(debug_knob("spgemm_lds_slots", kSpgemmLdsMax), kSpgemmMinSlots, kSpgemmLdsMax);
    const uint32_t wave_slots = std::min(lds_slots, spgemm_pow2_floor(debug_knob("spgemm_wave_slots", kSpgemmWaveMax), kSpgemmMinSlots, kSpgemmWaveMax));
    a->spgemm_lds_slots = use_lds ? lds_slots : 0u;
    a->spgemm_wave_slots = use_wave ? wave_slots : 0u;
    uint32_t group = 4;
    while (group < 64u && (uint64_t)group * n < b->nnz) group <<= 1;
    const long forced = debug_knob("spgemm_group", 0);
    a->spgemm_group = forced > 0 ? spgemm_pow2_floor(forced, 1u, 64u) : group;
    if (fresh) GL_HIP(hipMemsetAsync(m.compact, 0, 4, s));                    // gl_compact.h's ticket
    spgemm_zero_kernel<<<1, 256, 0, s>>>(m.bound, 0u, m.ctl);
    GL_LAUNCH_CHECK();
    spgemm_bound_kernel<<<rows_stream_grid(n), 256, 0, s>>>(a->d_csr_indptr, a->d_csr_indices, a->csr_nz_base, b->d_csr_indptr, n, m.bound, m.ctl);
    GL_LAUNCH_CHECK();
    if ((rc = spgemm_bin(a, m, 0, m.bound, nullptr)) != GL_OK) return rc;
    GL_HIP(hipStreamSynchronize(s));
    GL_HIP(hipMemcpy(&a->spgemm_products, m.ctl, 8, hipMemcpyDeviceToHost));
    if ((rc = spgemm_list_sizes(m, 0, a->spgemm_bins)) != GL_OK) return rc;
    if (a->spgemm_bins[2] && !a->d_spgemm_slab) {
        // a slab per RESIDENT workgroup, all zero between rows: the grid is capped so that the slabs stay inside the budget.  Their
        // number does not depend on this partner's slab rows: a later partner with more of them finds the same grid
        const uint64_t budget = (uint64_t)std::max<long>(0, std::min<long>(debug_knob("spgemm_scratch_mb", 1024), 1l << 20)) << 20;
        const uint64_t per_slab = 4ull * cdiv(n, 32u) + 8ull * n;
        const uint64_t slabs = std::min<uint64_t>(budget / per_slab, (uint64_t)ctx().num_cus);
        if (slabs == 0)
            return set_error(GL_ERR_UNSUPPORTED, "%s: a dense accumulator over %u columns takes %llu bytes, more than spgemm_scratch_mb allows (%llu bytes)",
                             who, n, (unsigned long long)per_slab, (unsigned long long)budget);
        const hipError_t e = hipMalloc((void **)&a->d_spgemm_slab, slabs * per_slab);
        if (e != hipSuccess) return set_error(GL_ERR_HIP, "%s: %llu slabs of %llu bytes: %s", who, (unsigned long long)slabs, (unsigned long long)per_slab, hipGetErrorString(e));
        GL_HIP(hipMemsetAsync(a->d_spgemm_slab, 0, slabs * per_slab, s));
        a->spgemm_slabs = (uint32_t)slabs;
    }
    a->spgemm_partner = b;
    a->spgemm_partner_uid = b->uid;
    return GL_OK;
}

template <int MODE, bool WG>
static int spgemm_launch_hash(const SpgemmArgs &g, unsigned grid, hipStream_t s) {
    const unsigned threads = WG ? kSpgemmThreads : kSpgemmWaveThreads;
    const size_t agents = WG ? 1u : threads / 64u;
    const size_t lds = (MODE >= kSpgemmMulAdd ? 8u * agents * g.tmax : 0u) + 8u * 17u + 4u * agents * g.tmax + 4u +
                       (WG && g.mask_mode ? 4u * kSpgemmMaskStage : 0u);
    if (lds > kSpgemmLdsOptIn) {
        static int attr_device = -1;   // per template instantiation; the opt-in is per device (gl_init may switch devices)
        if (attr_device != ctx().device) {
            GL_HIP(hipFuncSetAttribute((const void *)spgemm_hash_kernel<MODE, WG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
            attr_device = ctx().device;
        }
    }
    spgemm_hash_kernel<MODE, WG><<<grid, threads, lds, s>>>(g);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// the three paths over the lists `first` .. `first + 2`; most[b] = an upper bound of the rows in list b known to the host
template <int MODE>
static int spgemm_run(gl_spmv_plan a, SpgemmArgs g, const SpgemmScratch &m, int first, const uint32_t (&most)[3]) {
    hipStream_t s = ctx().stream;
    // A/B knob (GRAPHLILY_DEBUG, read per call): spgemm_grid = workgroups per compute unit of the wavefront path (a guess)
    const unsigned per_cu = (unsigned)std::max<long>(1, std::min<long>(debug_knob("spgemm_grid", 8), 1024));
    const unsigned cus = (unsigned)ctx().num_cus;
    int rc = GL_OK;
    if (most[0] && a->spgemm_wave_slots) {
        g.items = m.list[first];
        g.tmax = a->spgemm_wave_slots;
        rc = spgemm_launch_hash<MODE, false>(g, std::min(cdiv(most[0], kSpgemmWaveThreads / 64u), cus * per_cu), s);
    }
    if (rc == GL_OK && most[1] && a->spgemm_lds_slots) {
        g.items = m.list[first + 1];
        g.tmax = a->spgemm_lds_slots;
        rc = spgemm_launch_hash<MODE, true>(g, std::min(most[1], cus * 2u), s);
    }
    if (rc == GL_OK && most[2] && a->spgemm_slabs) {
        g.items = m.list[first + 2];
        g.slab_words = cdiv(g.n, 32u);
        g.slab_bits = reinterpret_cast<uint32_t *>(a->d_spgemm_slab + 8ull * g.n * a->spgemm_slabs);
        g.slab_val = reinterpret_cast<unsigned long long *>(a->d_spgemm_slab);
        spgemm_slab_kernel<MODE><<<std::min(most[2], a->spgemm_slabs), kSpgemmThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    return rc;
}

// the refusals of both calls; *empty: C has no entries whatever the values (*no_products: because an operand has none); the
// mask mode the kernels get
static int spgemm_require(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t flags, const char *who, bool *empty, bool *no_products,
                          uint32_t *mask_mode) {
    if (flags & ~GL_SPGEMM_MASK_COMPLEMENT) return set_error(GL_ERR_INVALID_ARG, "%s: flags 0x%x", who, flags);
    if ((flags & GL_SPGEMM_MASK_COMPLEMENT) && !mask) return set_error(GL_ERR_INVALID_ARG, "%s: GL_SPGEMM_MASK_COMPLEMENT without a mask", who);
    int rc = rows_require(a, kRowsSets, who, "plan a", "io.sort_rows_simple");
    if (rc == GL_OK && b != a) rc = rows_require(b, kRowsSets, who, "plan b", "io.sort_rows_simple");
    if (rc == GL_OK && mask && mask != a && mask != b) rc = rows_require(mask, kRowsSets, who, "the mask", "io.sort_rows_simple");
    if (rc != GL_OK) return rc;
    if (b->num_rows != a->num_rows || (mask && mask->num_rows != a->num_rows))
        return set_error(GL_ERR_UNSUPPORTED, "%s: the plans are over %u, %u and %u vertices: rectangular operands are out of scope", who, a->num_rows,
                         b->num_rows, mask ? mask->num_rows : a->num_rows);
    const bool complement = (flags & GL_SPGEMM_MASK_COMPLEMENT) != 0;
    *mask_mode = !mask ? 0u : mask->nnz == 0 ? (complement ? 0u : 1u) : complement ? 2u : 1u;
    *no_products = a->nnz == 0 || b->nnz == 0;
    *empty = *no_products || (mask && mask->nnz == 0 && !complement);
    return GL_OK;
}

static SpgemmArgs spgemm_args(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t mask_mode) {
    SpgemmArgs g = {};
    g.a_ptr = a->d_csr_indptr;
    g.a_idx = a->d_csr_indices;
    g.a_base = a->csr_nz_base;
    g.b_ptr = b->d_csr_indptr;
    g.b_idx = b->d_csr_indices;
    g.b_base = b->csr_nz_base;
    if (mask_mode) {
        g.m_ptr = mask->d_csr_indptr;
        g.m_idx = mask->d_csr_indices;
        g.m_base = mask->csr_nz_base;
    }
    g.n = a->num_rows;
    g.group = a->spgemm_group;
    g.mask_mode = mask_mode;
    return g;
}

static int spgemm_symbolic(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t flags, uint32_t *d_c_indptr, uint64_t *h_stats,
                           const char *who) {
    bool empty = false, no_products = false;
    uint32_t mask_mode = 0;
    int rc = spgemm_require(a, b, mask, flags, who, &empty, &no_products, &mask_mode);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = a->num_rows;
    h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0;
    if (!no_products && (rc = spgemm_prepare(a, b, who)) != GL_OK) return rc;      // (a mask without entries leaves the products as they are)
    spgemm_zero_kernel<<<rows_stream_grid(n + 1u), 256, 0, s>>>(d_c_indptr, n + 1u, nullptr);
    GL_LAUNCH_CHECK();
    if (!no_products) h_stats[1] = a->spgemm_products;
    if (empty || a->spgemm_products == 0) {
        GL_HIP(hipStreamSynchronize(s));
        return GL_OK;
    }
    SpgemmScratch m;
    spgemm_scratch_map(a->d_spgemm_scratch, n, &m);
    SpgemmArgs g = spgemm_args(a, b, mask, mask_mode);
    g.bound = m.bound;
    g.counts = d_c_indptr;
    if ((rc = spgemm_run<kSpgemmSymbolic>(a, g, m, 0, a->spgemm_bins)) != GL_OK) return rc;
    spgemm_offsets_kernel<<<1, 1024, 0, s>>>(d_c_indptr, n, m.ctl + 1);
    GL_LAUNCH_CHECK();
    GL_HIP(hipStreamSynchronize(s));
    unsigned long long nnz = 0;
    GL_HIP(hipMemcpy(&nnz, m.ctl + 1, 8, hipMemcpyDeviceToHost));
    h_stats[0] = nnz;
    h_stats[1] = a->spgemm_products;
    h_stats[2] = a->spgemm_bins[1];
    h_stats[3] = a->spgemm_bins[2];
    if (nnz > 0xffffffffull)
        return set_error(GL_ERR_UNSUPPORTED, "%s: C has %llu entries, which do not fit 32-bit offsets", who, nnz);
    return GL_OK;
}

static int spgemm_numeric(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t flags, uint32_t semiring, const float *d_a_val,
                          const float *d_b_val, const uint32_t *d_c_indptr, uint32_t *d_c_indices, float *d_c_val, uint64_t *h_stats, const char *who) {
    bool empty = false, no_products = false;
    uint32_t mask_mode = 0;
    int rc = spgemm_require(a, b, mask, flags, who, &empty, &no_products, &mask_mode);
    if (rc != GL_OK) return rc;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0;
    if (no_products) return GL_OK;
    if ((rc = spgemm_prepare(a, b, who)) != GL_OK) return rc;
    if (h_stats) h_stats[1] = a->spgemm_products;
    if (empty || a->spgemm_products == 0) return GL_OK;
    const uint32_t n = a->num_rows;
    SpgemmScratch m;
    spgemm_scratch_map(a->d_spgemm_scratch, n, &m);
    if ((rc = spgemm_bin(a, m, 3, nullptr, d_c_indptr)) != GL_OK) return rc;
    SpgemmArgs g = spgemm_args(a, b, mask, mask_mode);
    g.a_val = d_a_val;
    g.b_val = d_b_val;
    g.c_ptr = d_c_indptr;
    g.c_idx = d_c_indices;
    g.c_val = d_c_val;
    // |C(i)| <= the row's bound, so a list by |C(i)| holds no more rows than the symbolic lists from its own path upwards
    const uint32_t *sb = a->spgemm_bins;
    const uint32_t most[3] = {sb[0] + sb[1] + sb[2], sb[1] + sb[2], sb[2]};
    rc = semiring == GL_OP_MULADD   ? spgemm_run<kSpgemmMulAdd>(a, g, m, 3, most)
         : semiring == GL_OP_ADDMIN ? spgemm_run<kSpgemmAddMin>(a, g, m, 3, most)
                                    : spgemm_run<kSpgemmPattern>(a, g, m, 3, most);
    if (rc != GL_OK || !h_stats) return rc;
    GL_HIP(hipStreamSynchronize(ctx().stream));
    uint32_t sizes[3] = {0, 0, 0}, nnz = 0;
    if ((rc = spgemm_list_sizes(m, 3, sizes)) != GL_OK) return rc;
    GL_HIP(hipMemcpy(&nnz, d_c_indptr + n, 4, hipMemcpyDeviceToHost));
    h_stats[0] = nnz;
    h_stats[1] = a->spgemm_products;
    h_stats[2] = sizes[1];
    h_stats[3] = sizes[2];
    return GL_OK;
}

}  // namespace gl

int gl_spgemm_symbolic(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t flags, uint32_t *d_c_indptr, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(a != nullptr && b != nullptr && d_c_indptr != nullptr && h_stats != nullptr);
    return gl::spgemm_symbolic(a, b, mask, flags, d_c_indptr, h_stats, "gl_spgemm_symbolic");
}

int gl_spgemm_numeric(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t flags, uint32_t semiring, const float *d_a_val,
                      const float *d_b_val, const uint32_t *d_c_indptr, uint32_t *d_c_indices, float *d_c_val, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(a != nullptr && b != nullptr && d_c_indptr != nullptr && d_c_indices != nullptr);
    GL_ARG(semiring == GL_OP_MULADD || semiring == GL_OP_ANDOR || semiring == GL_OP_ADDMIN);
    GL_ARG(semiring == GL_OP_ANDOR || (d_a_val != nullptr && d_b_val != nullptr && d_c_val != nullptr));
    return gl::spgemm_numeric(a, b, mask, flags, semiring, d_a_val, d_b_val, d_c_indptr, d_c_indices, d_c_val, h_stats, "gl_spgemm_numeric");
}
