// The lock-free union-find of gl_cc.hip, for the two files that unite vertices in one launch and flatten the forest behind it:
// gl_cc.hip (weak components) and gl_bicc.hip (the blocks of the tree edges, the 2-edge-connected components).  gl_cc.hip's header
// states THE INVARIANT (parent[x] <= x, chains strictly descend) and the discipline (parent[] is atomic-only inside the uniting
// launch; a failed compare-and-swap goes on from the value it returned); the code here is that file's, moved unchanged.
#ifndef GL_UNIONFIND_H_
#define GL_UNIONFIND_H_

#include "gl_rounds.h"

namespace gl {

constexpr uint32_t kCcMaxRounds = 36;      // ceil(log2 2^32) + 1, made odd, with room
constexpr uint32_t kCcCtlBytes = 256;      // one "changed" word per finish round

// the root below x (as far as this thread's loads can tell); every vertex passed on the way is pointed at its grandparent
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t x) {
    uint32_t p = ga_load(parent + x);
    while (p < x) {
        const uint32_t g = ga_load(parent + p);
        if (g < p) ga_min(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// unite the components of a and b (a is an ancestor-or-self of the row's vertex); -> the row's new ancestor
__device__ __forceinline__ uint32_t cc_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return a;
        const uint32_t hi = max(a, b), lo = min(a, b);
        uint32_t seen = hi;
        if (ga_cas(parent + hi, seen, lo)) return lo;
        // hi was hooked by somebody else meanwhile: go on from where it points now (seen < hi)
        if (a == hi) a = seen;
        else b = seen;
    }
}

// one round of pointer doubling: out[v] = in[in[v]]; changed[round] != 0 if some vertex moved.  A round whose predecessor
// changed nothing returns at once: in == out already, element for element.
static __global__ __launch_bounds__(256) void cc_jump_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n,
                                                             uint32_t *__restrict__ changed, uint32_t round) {
    if (round != 0u && changed[round - 1u] == 0u) return;
    bool moved = false;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t p = in[v], g = in[p];
        out[v] = g;
        moved |= g != p;
    }
    if (__any(moved) && (threadIdx.x & 63u) == 0u) atomicOr(changed + round, 1u);
}

// Pointer doubling behind the uniting launch (plain loads), n >= 1: ping-pong between d_parent and d_labels, an odd number of
// rounds, so that the last one writes d_labels[v] = the root of v, the smallest vertex of its class.  No synchronisation.
static int cc_double(uint32_t *d_parent, uint32_t n, uint32_t *d_labels, const char *who) {
    hipStream_t s = ctx().stream;
    uint32_t *&ctl = ctx().cc_ctl;
    const int rc = plan_scratch(ctl, kCcCtlBytes, who, "control words");
    if (rc != GL_OK) return rc;
    GL_HIP(hipMemsetAsync(ctl, 0, kCcCtlBytes, s));
    uint32_t rounds = 1;                      // ceil(log2 n) + 1 ...
    while ((1ull << (rounds - 1u)) < n) rounds++;
    rounds |= 1u;                             // ... made odd: the last round writes d_labels
    static_assert(kCcMaxRounds * 4u <= kCcCtlBytes && kCcMaxRounds >= 33u, "one word per round");
    const unsigned grid = rows_stream_grid(n);
    uint32_t *in = d_parent, *out = d_labels;
    for (uint32_t r = 0; r < rounds; r++) {
        cc_jump_kernel<<<grid, 256, 0, s>>>(in, out, n, ctl, r);
        GL_LAUNCH_CHECK();
        std::swap(in, out);
    }
    return GL_OK;
}

// gl_cc.hip: parent[v] = v, and the hook of every row of a plan that passed kRowsIndexable into `d_parent`
int cc_begin(uint32_t *d_parent, uint32_t n);
int cc_hook(gl_spmv_plan p, uint32_t *d_parent);

}  // namespace gl

#endif  // GL_UNIONFIND_H_
