// What the kernels that keep a label per vertex and sweep the vertices colour class by colour class share -- gl_lpa and
// gl_louvain_move --, stated once: the words of the control record that the colour bucketing writes, the bucketing itself (the
// check of the colouring with the histogram, the scan, the scatter: list and offs), the hash of the label tables and the
// wavefront helpers around a wavefront's own LDS table.  The kernels are static: each of the two files launches its own copy.
#ifndef GL_CLASSES_H_
#define GL_CLASSES_H_

#include "gl_rounds.h"

namespace gl {

// the words of the second 128-byte line of a control record that the bucketing adds to (each caller's record keeps them here)
enum : uint32_t { kLpaTop = 33, kLpaBadColor = 39, kLpaImproper = 40 };
constexpr uint32_t kLpaEmpty = 0xffffffffu;      // the empty key of a slot: no label
constexpr uint32_t kLpaProbes = 16;              // slots a label tries before its row overflows
constexpr uint32_t kLpaHistBins = 1024;          // colours a workgroup of the check counts in LDS
constexpr uint32_t kLpaCheckCut = 32;            // entries of a row that the check reads in one thread (as gl_color's init)
constexpr uint32_t kLpaMaxParts = 1u << 20;

__device__ __forceinline__ uint32_t lpa_wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += __shfl_xor(x, d);
    return x;
}

// one launch over the entries: colours >= n, entries whose two ends share a colour, the histogram of the colours and the largest
static __global__ __launch_bounds__(256) void lpa_check_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                        const uint32_t *__restrict__ color, uint32_t n, uint32_t nz_base,
                                                        uint32_t *hist, uint32_t *ctl) {
    __shared__ uint32_t bins[kLpaHistBins];
    for (uint32_t i = threadIdx.x; i < kLpaHistBins; i += 256u) bins[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t top = 0, bad = 0, improper = 0;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        uint32_t beg = 0, end = 0, cv = kLpaEmpty;
        if (v64 < n) {
            cv = color[v];
            if (cv >= n) {
                bad += 1u;
                cv = kLpaEmpty;
            } else {
                if (cv < kLpaHistBins) atomicAdd(&bins[cv], 1u);
                else ga_add(hist + cv, 1u);
                top = max(top, cv);
                beg = row_ptr[v] - nz_base;
                end = row_ptr[v + 1u] - nz_base;
            }
        }
        if (end - beg <= kLpaCheckCut) {
            for (; beg < end; beg++) {
                const uint32_t u = row_idx[beg];
                if (u < n && u != v && color[u] == cv) improper += 1u;
            }
        }
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t row = __shfl(v, src), rc = __shfl(cv, src);
            rows_walk_wave(row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                uint32_t k[4];
#pragma unroll
                for (int u = 0; u < 4; u++) k[u] = (c[u] < n && c[u] != row) ? color[c[u]] : kLpaEmpty;
#pragma unroll
                for (int u = 0; u < 4; u++) improper += k[u] == rc ? 1u : 0u;      // (rc is a colour below n, never the empty key)
                return false;
            });
        });
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) top = max(top, (uint32_t)__shfl_xor(top, d));
    bad = lpa_wave_sum(bad);
    improper = lpa_wave_sum(improper);
    if (lane == 0u) {
        if (top != 0u) ga_max(ctl + kLpaTop, top);
        if (bad != 0u) ga_add(ctl + kLpaBadColor, bad);
        if (improper != 0u) ga_add(ctl + kLpaImproper, improper);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kLpaHistBins && i < n; i += 256u)
        if (bins[i] != 0u) ga_add(hist + i, bins[i]);
}

// ONE workgroup: offs[c] = the vertices of the colours below c, c = 0 .. classes; hist becomes the scatter's cursors
static __global__ __launch_bounds__(1024) void lpa_scan_kernel(uint32_t *__restrict__ hist, uint32_t *__restrict__ offs, const uint32_t *ctl, uint32_t n) {
    __shared__ uint32_t wsum[16];
    const uint32_t classes = min(ctl[kLpaTop], n - 1u) + 1u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t run = 0;
    for (uint64_t base = 0; base < classes; base += 1024u) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t x = i < classes ? hist[i] : 0u;
        uint32_t incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if ((int)lane >= d) incl += t;
        }
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 16u; w++) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        const uint32_t excl = run + before + incl - x;
        if (i < classes) {
            offs[i] = excl;
            hist[i] = excl;
        }
        run += total;
        __syncthreads();
    }
    if (threadIdx.x == 0u) offs[classes] = run;
}

static __global__ __launch_bounds__(256) void lpa_scatter_kernel(const uint32_t *__restrict__ color, uint32_t n, uint32_t *cursor, uint32_t *__restrict__ list) {
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < n; v64 += gridDim.x * 256u) {
        const uint32_t cv = color[v64];
        if (cv >= n) continue;
        const uint32_t pos = ga_add(cursor + cv, 1u);
        if (pos < n) list[pos] = (uint32_t)v64;                   // (pos < n: every vertex is scattered once)
    }
}

// Murmur3's finaliser, a bijection of the 32-bit words: the low bits pick the slot, the bits from 12 up the partition
__device__ __forceinline__ uint32_t lpa_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// what one lane stored in the wavefront's table, every lane may read behind this
__device__ __forceinline__ void lpa_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long lpa_wave_max(unsigned long long x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_xor(x, d);
        x = y > x ? y : x;
    }
    return x;
}

}  // namespace gl

#endif  // GL_CLASSES_H_
