// The outer iteration of PageRank.solve: the pass that follows each SpMV y = M x.
//
//   c        = (float)((1.0 - (double)d) + (double)d * dangle[slot - 1])
//   x_new[v] = fl32(y[v] + fl32(c * p[v]))                         (a float multiply, then a float add: never fused)
//   r[slot]      = sum over v of |(double)x_new[v] - (double)x[v]|
//   dangle[slot] = sum over the dangling v of (double)x_new[v]      (bit v % 32 of word v / 32 of the dangling bits)
//
// x_new goes over y, the two sums stay on the device in the control block (graphlily_hip.h), and an update whose residual is
// <= tol sets `done`: every update enqueued after it copies x to its output and changes nothing else, so the host may enqueue
// several iterations ahead and read the few control words back once per batch.
//
// Pure streaming, 16 n + n / 8 bytes: an item is four consecutive elements (one 16-byte load of y, x and p per lane, one
// 16-byte store; the dangling word of an item is shared by eight neighbouring lanes), grid-stride.  The sums are
// DETERMINISTIC: the number of workgroups depends on n alone (never on the device or on the pointers' alignment -- the
// scalar path walks the same items in the same order), a thread adds its items in ascending order, a workgroup combines its
// 256 sums in one fixed shape and stores ONE f64 pair, and a one-workgroup launch behind it adds the pairs in workgroup-index
// order (two threads, one per sum) -- no floating-point atomics, and no hand-off inside a launch: the launch boundary
// publishes the partials.  No call synchronises with the host; everything is enqueued on the library's stream.
#include "gl_common.h"

#include <algorithm>

namespace gl {

constexpr uint32_t kPrThreads = 256;
constexpr uint32_t kPrMaxGroups = GL_PAGERANK_MAX_GROUPS;
constexpr uint32_t kPrHeadWords = 4;     // {done, iterations, slots, 0}

static_assert(kPrMaxGroups * 16u <= 32768u, "the finishing workgroup keeps every partial pair in LDS");

// a function of n alone
static inline uint32_t pr_groups(uint32_t n) { return std::max(1u, std::min<uint32_t>(cdiv(cdiv(n, 4), kPrThreads), kPrMaxGroups)); }

static inline size_t pr_head_bytes(uint32_t slots) { return kPrHeadWords * 4u + 16u * ((size_t)slots + 1u); }

struct PrCtl {
    uint32_t *head;
    double *dangle, *residual, *partial;
};

__host__ __device__ __forceinline__ PrCtl pr_ctl(void *ctl, uint32_t slots) {
    PrCtl c;
    c.head = (uint32_t *)ctl;
    c.dangle = (double *)(c.head + kPrHeadWords);
    c.residual = c.dangle + (slots + 1u);
    c.partial = c.residual + (slots + 1u);
    return c;
}

struct PrArgs {
    float *out;               // update: y in, x_new out; begin: x
    const float *x, *p;
    const uint32_t *bits;
    void *ctl;
    uint32_t n, slot;         // begin: slot = slots
    float damping;
};

// the workgroup's two sums, in one fixed shape, into its partial pair
__device__ __forceinline__ void pr_store_partials(double r, double dg, double *partial) {
    __shared__ double wave_sums[2][kPrThreads / 64];
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        r += __shfl_down(r, off);
        dg += __shfl_down(dg, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
        wave_sums[0][threadIdx.x >> 6] = r;
        wave_sums[1][threadIdx.x >> 6] = dg;
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        const double *s = wave_sums[threadIdx.x];
        partial[2u * blockIdx.x + threadIdx.x] = ((s[0] + s[1]) + s[2]) + s[3];
    }
}

// out = src over the items of this grid (begin: x = p; a frozen update: y = x)
template <bool VEC>
__device__ __forceinline__ void pr_copy_item(float *out, const float *src, uint32_t i, uint32_t n, float (&v)[4]) {
    if (VEC && i < (n >> 2)) {
        const float4 q = reinterpret_cast<const float4 *>(src)[i];
        reinterpret_cast<float4 *>(out)[i] = q;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t e = 4u * i + k;      // (i < ceil(n / 4): 4 i + k < n + 3 fits)
            v[k] = 0.0f;
            if (e < n) out[e] = v[k] = src[e];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void pagerank_begin_kernel(PrArgs a) {
    const uint32_t items = (a.n >> 2) + ((a.n & 3u) ? 1u : 0u), stride = gridDim.x * kPrThreads;
    double dg = 0.0;
    for (uint32_t i = blockIdx.x * kPrThreads + threadIdx.x; i < items; i += stride) {
        const uint32_t w = a.bits[i >> 3] >> ((i & 7u) * 4u);
        float v[4];
        pr_copy_item<VEC>(a.out, a.p, i, a.n, v);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            if (((w >> k) & 1u) && 4u * i + k < a.n) dg += (double)v[k];
    }
    pr_store_partials(0.0, dg, pr_ctl(a.ctl, a.slot).partial);
}

template <bool VEC>
__global__ __launch_bounds__(256) void pagerank_update_kernel(PrArgs a) {
#pragma clang fp contract(off)
    const uint32_t items = (a.n >> 2) + ((a.n & 3u) ? 1u : 0u), stride = gridDim.x * kPrThreads;
    const uint32_t first = blockIdx.x * kPrThreads + threadIdx.x;
    const uint32_t *head = (const uint32_t *)a.ctl;
    const uint32_t slots = head[2];
    // converged before this slot, or no such slot (or a block gl_pagerank_begin never saw): the vector stays in place
    if (head[0] != 0u || a.slot > slots || slots > GL_PAGERANK_MAX_SLOTS) {
        float v[4];
        for (uint32_t i = first; i < items; i += stride) pr_copy_item<VEC>(a.out, a.x, i, a.n, v);
        return;
    }
    const PrCtl ctl = pr_ctl(a.ctl, slots);
    const double d = (double)a.damping;
    const double scaled = d * ctl.dangle[a.slot - 1u];
    const float c = (float)((1.0 - d) + scaled);
    double r = 0.0, dg = 0.0;
#pragma unroll 2
    for (uint32_t i = first; i < items; i += stride) {
        const uint32_t w = a.bits[i >> 3] >> ((i & 7u) * 4u);
        float y[4], x[4], p[4];
        const bool full = VEC && i < (a.n >> 2);
        if (full) {
            const float4 yq = reinterpret_cast<const float4 *>(a.out)[i];
            const float4 xq = reinterpret_cast<const float4 *>(a.x)[i];
            const float4 pq = reinterpret_cast<const float4 *>(a.p)[i];
            y[0] = yq.x; y[1] = yq.y; y[2] = yq.z; y[3] = yq.w;
            x[0] = xq.x; x[1] = xq.y; x[2] = xq.z; x[3] = xq.w;
            p[0] = pq.x; p[1] = pq.y; p[2] = pq.z; p[3] = pq.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t e = 4u * i + k;
                const bool in = e < a.n;
                y[k] = in ? a.out[e] : 0.0f;
                x[k] = in ? a.x[e] : 0.0f;
                p[k] = in ? a.p[e] : 0.0f;
            }
        }
        float xn[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const float t = c * p[k];
            xn[k] = y[k] + t;
        }
        if (full) {
            reinterpret_cast<float4 *>(a.out)[i] = make_float4(xn[0], xn[1], xn[2], xn[3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                if (4u * i + k < a.n) a.out[4u * i + k] = xn[k];
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            if (full || 4u * i + k < a.n) {
                r += fabs((double)xn[k] - (double)x[k]);
                if ((w >> k) & 1u) dg += (double)xn[k];
            }
        }
    }
    pr_store_partials(r, dg, ctl.partial);
}

// one workgroup behind the pass: the partial pairs in workgroup-index order, one thread per sum
template <bool BEGIN>
__global__ __launch_bounds__(256) void pagerank_finish_kernel(void *ctl_ptr, uint32_t groups, uint32_t slot, double tol) {
    __shared__ double pairs[2u * kPrMaxGroups];
    uint32_t *head = (uint32_t *)ctl_ptr;
    const uint32_t slots = BEGIN ? slot : head[2];
    if (!BEGIN && (head[0] != 0u || slot > slots || slots > GL_PAGERANK_MAX_SLOTS)) return;    // (uniform; read before the barrier, written after it)
    const PrCtl ctl = pr_ctl(ctl_ptr, slots);
    for (uint32_t i = threadIdx.x; i < 2u * groups; i += kPrThreads) pairs[i] = ctl.partial[i];
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (BEGIN) {
            head[2] = slots;
        } else {
            double r = 0.0;
            for (uint32_t g = 0; g < groups; g++) r += pairs[2u * g];
            ctl.residual[slot] = r;
            head[1] = slot;
            if (r <= tol) head[0] = 1u;
        }
    } else if (threadIdx.x == 64u) {      // (another wavefront: the two chains run side by side)
        double dg = 0.0;
        for (uint32_t g = 0; g < groups; g++) dg += pairs[2u * g + 1u];
        ctl.dangle[BEGIN ? 0u : slot] = dg;
    }
}

static inline bool pr_aligned16(const void *a, const void *b, const void *c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

}  // namespace gl

extern "C" {

int gl_pagerank_ctl_bytes(uint32_t slots, size_t *bytes) {
    GL_ARG(bytes != nullptr && slots >= 1u && slots <= GL_PAGERANK_MAX_SLOTS);
    *bytes = gl::pr_head_bytes(slots) + 16u * (size_t)gl::kPrMaxGroups;
    return GL_OK;
}

int gl_pagerank_begin(const float *d_p, uint32_t n, const uint32_t *d_dangling_bits, float *d_x, void *d_ctl, uint32_t slots) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(d_p != nullptr && d_dangling_bits != nullptr && d_x != nullptr && d_ctl != nullptr && d_x != d_p);
    GL_ARG(n >= 1u && slots >= 1u && slots <= GL_PAGERANK_MAX_SLOTS && ((uintptr_t)d_ctl & 7u) == 0);
    hipStream_t s = gl::ctx().stream;
    GL_HIP(hipMemsetAsync(d_ctl, 0, gl::pr_head_bytes(slots), s));
    gl::PrArgs a;
    a.out = d_x;
    a.x = nullptr;
    a.p = d_p;
    a.bits = d_dangling_bits;
    a.ctl = d_ctl;
    a.n = n;
    a.slot = slots;
    a.damping = 0.0f;
    const uint32_t groups = gl::pr_groups(n);
    if (gl::pr_aligned16(d_x, d_p, nullptr)) gl::pagerank_begin_kernel<true><<<groups, gl::kPrThreads, 0, s>>>(a);
    else gl::pagerank_begin_kernel<false><<<groups, gl::kPrThreads, 0, s>>>(a);
    GL_LAUNCH_CHECK();
    gl::pagerank_finish_kernel<true><<<1, gl::kPrThreads, 0, s>>>(d_ctl, groups, slots, 0.0);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pagerank_update(float *d_y_inout, const float *d_x, const float *d_p, const uint32_t *d_dangling_bits, uint32_t n,
                       float damping, double tol, void *d_ctl, uint32_t slot) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(d_y_inout != nullptr && d_x != nullptr && d_p != nullptr && d_dangling_bits != nullptr && d_ctl != nullptr);
    GL_ARG(d_y_inout != d_x && d_y_inout != d_p && n >= 1u && ((uintptr_t)d_ctl & 7u) == 0);
    if (slot < 1u || slot > GL_PAGERANK_MAX_SLOTS)
        return gl::set_error(GL_ERR_INVALID_ARG, "gl_pagerank_update: slot %u is not in [1, %u]", slot, GL_PAGERANK_MAX_SLOTS);
    hipStream_t s = gl::ctx().stream;
    gl::PrArgs a;
    a.out = d_y_inout;
    a.x = d_x;
    a.p = d_p;
    a.bits = d_dangling_bits;
    a.ctl = d_ctl;
    a.n = n;
    a.slot = slot;
    a.damping = damping;
    const uint32_t groups = gl::pr_groups(n);
    if (gl::pr_aligned16(d_y_inout, d_x, d_p)) gl::pagerank_update_kernel<true><<<groups, gl::kPrThreads, 0, s>>>(a);
    else gl::pagerank_update_kernel<false><<<groups, gl::kPrThreads, 0, s>>>(a);
    GL_LAUNCH_CHECK();
    gl::pagerank_finish_kernel<false><<<1, gl::kPrThreads, 0, s>>>(d_ctl, groups, slot, tol);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"

// gl_init loads this translation unit's code object up front (HIP defers that to the unit's first launch)
namespace gl {
int preload_pagerank() {
    hipFuncAttributes attr;
    GL_HIP(hipFuncGetAttributes(&attr, (const void *)pagerank_finish_kernel<false>));
    return GL_OK;
}
}  // namespace gl
