// Betweenness centrality (gl_bc_accumulate): Brandes' dependency accumulation of ONE finished search, level-synchronous, over the
// plain CSR copies that GL_PLAN_BOOLEAN plans keep (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base).  plan_in's row v
// lists the vertices v is pulled from (an entry A[v,u] is the edge u -> v, the convention of the BFS drivers and gl_bfs_parents),
// plan_out's row u the out-neighbours of u (the transposed pattern; the same handle for a symmetric pattern).  Both are square,
// whole-matrix plans whose rows are strictly ascending sets of columns below n = num_rows.  `level` is the drivers' level array
// (1 on a source, it + 1 on a vertex reached in iteration it, 0 unreached), D = max level, all arithmetic in f64:
//
//   sigma[v] = 1 (level 1);  sum over u in row_in(v) with level[u] == level[v] - 1 of sigma[u] (level >= 2);  0 (level 0)
//   delta[u] = sigma[u] * sum over v in row_out(u) with level[v] == level[u] + 1 and sigma[v] > 0 of (1 + delta[v]) / sigma[v]
//   bc[u]    = (accumulate ? bc[u] : 0) + scale * delta[u]   for level[u] >= 2;   (accumulate ? bc[u] : 0)   otherwise
//
// THE CALL:
//   bucket    a histogram of the levels, an exclusive scan (one workgroup), a scatter of the vertex numbers into a level-ordered
//             QUEUE of n words -- one atomic per wavefront and distinct level.  The host waits ONCE here and reads D and the D + 2
//             offsets back to page-locked memory: the sweeps' launches are sized from them.
//   forward   levels 2 .. D, one launch per level over that level's queue slice, pulling sigma through plan_in
//   backward  levels D .. 2, one launch per level, pulling coef[v] = (1 + delta[v]) / sigma[v] through plan_out (an edge costs one
//             gather and one add, no division); the bc update is fused into the same launch.  Level D only stores its coef.
//             Every backward launch is gated by the count of non-finite sigmas on the device (path counts overflow f64 on
//             lattice-like graphs): bc then stays as accumulate ? bc : 0.
// The sweeps walk the rows of a level's queue slice, a thread per queued vertex, as gl_rows.h states the walk (a copy: see there).
// DETERMINISM: no floating-point atomics.  Every vertex's sum is formed by ONE owner in an order that depends only on the row and
// on bc_cut: the vertex's thread adds the first bc_cut entries in row order; a row still unfinished is taken over by its
// wavefront -- lane l adds the entries b + l, b + 64 + l, ... in that order, the 64 partial sums meet in a fixed xor tree -- and
// the thread adds that total to its own.  The order of the vertices inside a queue slice (an atomic cursor) changes no value.
// MEMORY RULES: inside one launch a vertex reads only values written by earlier launches (levels L -+ 1) and writes only its own
// words: plain loads and stores.  The counters (orphans, non-finite sigmas) are integer atomics, one per wavefront.  No spin-
// waits, no hand-offs between workgroups, no cooperative launch.
// GATHERS: an edge reads the neighbour's level (4 bytes) and, on a match only, its sigma / coef (8 bytes).  The packed 16-byte
// record per vertex that DESIGN.md 4.15 names as the alternative is NOT built.
#include "gl_rows.h"

namespace gl {

constexpr uint32_t kBcCtlBytes = 256;
constexpr uint32_t kBcFirstOffsets = 1024;   // offsets that travel with the control words in the one read-back (deeper: a second copy)
enum : uint32_t { kBcDepth = 0, kBcBadLevel = 1, kBcOrphans = 2, kBcNonFinite = 3, kBcCtlWords = 4 };

struct BcScratch {      // the plan's scratch, carved up
    uint32_t *ctl, *cursor, *off, *queue;
    double *sigma, *coef;
};

static size_t bc_scratch_bytes(uint32_t n) {
    const size_t words = 2u * ((size_t)n + 2u) + n;
    return kBcCtlBytes + ((words * 4u + 7u) & ~(size_t)7u) + 16u * (size_t)n;
}

static BcScratch bc_carve(unsigned char *base, uint32_t n) {
    BcScratch s;
    s.ctl = reinterpret_cast<uint32_t *>(base);
    s.cursor = s.ctl + kBcCtlBytes / 4u;
    s.off = s.cursor + ((size_t)n + 2u);
    s.queue = s.off + ((size_t)n + 2u);
    const size_t words = 2u * ((size_t)n + 2u) + n;
    s.sigma = reinterpret_cast<double *>(base + kBcCtlBytes + ((words * 4u + 7u) & ~(size_t)7u));
    s.coef = s.sigma + n;
    return s;
}

// a level as the drivers write it: a whole number 0 .. n
__device__ __forceinline__ bool bc_level_of(float f, uint32_t n, uint32_t *l) {
    const bool ok = f >= 0.0f && f <= (float)n && f == floorf(f) && (uint32_t)f <= n;
    *l = ok ? (uint32_t)f : 0u;
    return ok;
}

// every lane of the wavefront calls this; the active ones add 1 to counters[l] -- one atomic per distinct l -- and get the
// word's value before their own add
__device__ __forceinline__ uint32_t bc_wave_take(uint32_t *counters, uint32_t l, bool active, uint32_t lane) {
    uint32_t pos = 0;
    for (unsigned long long todo = __ballot(active); todo;) {
        const int leader = __ffsll(todo) - 1;
        const uint32_t ll = __shfl(l, leader);
        const bool mine = active && l == ll;
        const unsigned long long m = __ballot(mine);
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(counters + ll, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (mine) pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
    }
    return pos;
}

// hist[l] += 1 per vertex, D = max level, sigma = 1 on the sources and 0 elsewhere (levels >= 2 are overwritten by their sweep)
__global__ __launch_bounds__(256) void bc_hist_kernel(const float *__restrict__ level, uint32_t n, uint32_t *__restrict__ hist,
                                                      uint32_t *__restrict__ ctl, double *__restrict__ sigma) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;       // whole wavefronts take every trip
    uint32_t top = 0;
    bool bad = false;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u) {
        uint32_t l = 0;
        if (v < n) {
            bad |= !bc_level_of(level[v], n, &l);
            sigma[v] = l == 1u ? 1.0 : 0.0;
        }
        top = max(top, l);
        (void)bc_wave_take(hist, l, v < n, lane);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, o));
    if (lane == 0u && top != 0u) atomicMax(ctl + kBcDepth, top);
    if (__any(bad) && lane == 0u) atomicOr(ctl + kBcBadLevel, 1u);
}

// off[0 .. D + 1] = the exclusive scan of hist[0 .. D + 1] (hist[D + 1] is 0), and the scatter's cursors start there: ONE workgroup
__global__ __launch_bounds__(1024) void bc_scan_kernel(uint32_t *__restrict__ hist, uint32_t *__restrict__ off, const uint32_t *__restrict__ ctl) {
    __shared__ uint32_t part[1024];
    const uint32_t m = ctl[kBcDepth] + 2u, t = threadIdx.x;
    const uint32_t per = (m + 1023u) / 1024u;
    const uint64_t b = (uint64_t)t * per, e = min((uint64_t)m, b + per);
    uint32_t sum = 0;
    for (uint64_t i = b; i < e; i++) sum += hist[i];
    part[t] = sum;
    __syncthreads();
    if (t == 0u) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 1024u; i++) {
            const uint32_t x = part[i];
            part[i] = run;
            run += x;
        }
    }
    __syncthreads();
    uint32_t run = part[t];
    for (uint64_t i = b; i < e; i++) {
        const uint32_t x = hist[i];
        off[i] = run;
        hist[i] = run;
        run += x;
    }
}

__global__ __launch_bounds__(256) void bc_scatter_kernel(const float *__restrict__ level, uint32_t n, uint32_t *__restrict__ cursor,
                                                         uint32_t *__restrict__ queue) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u) {
        uint32_t l = 0;
        if (v < n) (void)bc_level_of(level[v], n, &l);
        const uint32_t pos = bc_wave_take(cursor, l, v < n, lane);
        if (v < n && pos < n) queue[pos] = (uint32_t)v;           // (pos < n: every vertex is counted once)
    }
}

struct BcSweepArgs {
    const uint32_t *row_ptr, *row_idx;     // plan_in (forward) or plan_out (backward)
    const float *level;
    const uint32_t *queue;                 // this level's slice
    uint32_t *ctl;
    double *sigma, *coef, *bc;
    double scale;
    float want;                            // the neighbours' level: L - 1 (forward), L + 1 (backward)
    uint32_t count, n, nz_base, cut_steps;
    uint32_t walk;                         // backward: 0 on level D, which has nobody below it
};

// one neighbour: its level first, the double only on a match
__device__ __forceinline__ double bc_gather(const float *__restrict__ level, const double *__restrict__ val, uint32_t u, float want) {
    return level[u] == want ? val[u] : 0.0;
}

template <bool FORWARD>
__global__ __launch_bounds__(256) void bc_sweep_kernel(BcSweepArgs a) {
    if (!FORWARD && a.ctl[kBcNonFinite] != 0u) return;            // (written by the forward launches: all behind us)
    const double *val = FORWARD ? a.sigma : a.coef;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (a.count + 63u) >> 6;
    uint32_t orphans = 0, nonfinite = 0;                          // per wavefront
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += gridDim.x * 4u) {
        const uint32_t item = wd * 64u + lane;
        const bool in = item < a.count;
        uint32_t v = 0, beg = 0, end = 0;
        if (in) {
            v = a.queue[item];
            if (FORWARD || a.walk != 0u) {
                beg = a.row_ptr[v] - a.nz_base;
                end = a.row_ptr[v + 1u] - a.nz_base;
            }
        }
        double acc = 0.0;
        // the walk of gl_rows.h in a copy of this kernel's own (through rows_walk_* the sweeps were 1 - 2 % slower on one stand-in
        // in two visits, EXPERIMENTS.md Round 21): the same wrap-free forms, the same padding column
        for (uint32_t step = 0; step < a.cut_steps && __any(beg < end); step++) {
            if (beg < end) {
                uint32_t c[4];
#pragma unroll
                for (int u = 0; u < 4; u++) c[u] = end - beg > (uint32_t)u ? a.row_idx[beg + u] : 0xffffffffu;
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n) acc += bc_gather(a.level, val, c[u], a.want);
                beg += min(4u, end - beg);
            }
        }
        // rows still unfinished are taken over by the whole wavefront, 256 entries per step (coalesced index loads); the 64
        // partial sums meet in a fixed tree
        for (uint64_t pending = __ballot(beg < end); pending; pending &= pending - 1ull) {
            const int src = __ffsll((unsigned long long)pending) - 1;
            const uint32_t b = __shfl(beg, src), e = __shfl(end, src);
            double part = 0.0;
            for (uint64_t base = b; base < e; base += 256u) {
                uint32_t c[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint64_t j = base + 64u * u + lane;
                    c[u] = j < e ? a.row_idx[j] : 0xffffffffu;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n) part += bc_gather(a.level, val, c[u], a.want);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
            if ((int)lane == src) acc += part;
        }
        if (FORWARD) {
            if (in) a.sigma[v] = acc;
            orphans += (uint32_t)__popcll(__ballot(in && acc == 0.0));
            nonfinite += (uint32_t)__popcll(__ballot(in && !(acc <= 1.7976931348623157e308)));
        } else if (in) {
            const double sg = a.sigma[v];
            const double delta = sg * acc;
            a.coef[v] = sg > 0.0 ? (1.0 + delta) / sg : 0.0;
            a.bc[v] += a.scale * delta;
        }
    }
    if (FORWARD && lane == 0u) {
        if (orphans) atomicAdd(a.ctl + kBcOrphans, orphans);
        if (nonfinite) atomicAdd(a.ctl + kBcNonFinite, nonfinite);
    }
}

// the refusals and the verdicts (gl_rows.h: rows_require_pair, shared with gl_scc), then plan_in's scratch, on first use
static int bc_prepare(gl_spmv_plan pin, gl_spmv_plan pout, const char *who) {
    const int rc = rows_require_pair(pin, pout, who, "io.simple_pattern");
    if (rc != GL_OK) return rc;
    return plan_scratch(pin->d_bc_scratch, bc_scratch_bytes(pin->num_rows), who, "queue, offsets, sigma and coef");
}

static int bc_accumulate(gl_spmv_plan pin, gl_spmv_plan pout, const float *d_level, double *d_bc, double scale, int accumulate,
                         double *d_sigma, uint32_t *h_stats, const char *who) {
    int rc = bc_prepare(pin, pout, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = pin->num_rows;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0u;
    if (n == 0u) return GL_OK;
    // A/B knobs (GRAPHLILY_DEBUG, read per call): bc_cut = entries a thread adds before the wavefront takes the row over (8, the
    // k-core peel's value; on two stand-ins 0 was 12 - 17 % slower and 64 within 2 %: profiles/bc.jsonl, EXPERIMENTS.md Round
    // 14), bc_grid = workgroups per compute unit of a sweep launch (4: an unmeasured guess)
    const long cut = debug_knob("bc_cut", 8), per_cu = debug_knob("bc_grid", 4);
    auto shape_for = [&](uint32_t count) { return rows_walk_shape(count, cut, 1l << 30, per_cu); };   // (a launch per level)
    const BcScratch sc = bc_carve(pin->d_bc_scratch, n);
    double *sigma = d_sigma ? d_sigma : sc.sigma;
    // page-locked landing room of the read-backs: the control words, then the offsets
    const size_t first = std::min<size_t>((size_t)n + 2u, kBcFirstOffsets);
    auto pinned_room = [&](size_t words) -> hipError_t {
        if (pin->bc_pinned_words >= words) return hipSuccess;
        if (pin->h_bc_pinned) (void)hipHostFree(pin->h_bc_pinned);
        pin->h_bc_pinned = nullptr;
        pin->bc_pinned_words = 0;
        const hipError_t e = hipHostMalloc((void **)&pin->h_bc_pinned, words * 4u, hipHostMallocDefault);
        if (e == hipSuccess) pin->bc_pinned_words = words;
        return e;
    };
    GL_HIP(pinned_room(kBcCtlBytes / 4u + kBcFirstOffsets));
    // (ctl and both offset arrays are one stretch: zeroed together)
    GL_HIP(hipMemsetAsync(sc.ctl, 0, kBcCtlBytes + 8u * ((size_t)n + 2u), s));
    if (!accumulate) GL_HIP(hipMemsetAsync(d_bc, 0, 8u * (size_t)n, s));
    const unsigned stream_grid = rows_stream_grid(n);
    bc_hist_kernel<<<stream_grid, 256, 0, s>>>(d_level, n, sc.cursor, sc.ctl, sigma);
    bc_scan_kernel<<<1, 1024, 0, s>>>(sc.cursor, sc.off, sc.ctl);
    bc_scatter_kernel<<<stream_grid, 256, 0, s>>>(d_level, n, sc.cursor, sc.queue);
    GL_LAUNCH_CHECK();
    uint32_t *w = pin->h_bc_pinned;
    GL_HIP(hipMemcpyAsync(w, sc.ctl, kBcCtlBytes, hipMemcpyDeviceToHost, s));
    GL_HIP(hipMemcpyAsync(w + kBcCtlBytes / 4u, sc.off, first * 4u, hipMemcpyDeviceToHost, s));
    GL_HIP(hipStreamSynchronize(s));
    if (w[kBcBadLevel] != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: d_level holds a value that is no level (a whole number 0 .. %u)", who, n);
    const uint32_t D = w[kBcDepth];
    if ((size_t)D + 2u > first) {      // a deep search: the rest of the offsets
        GL_HIP(pinned_room(kBcCtlBytes / 4u + (size_t)D + 2u));
        w = pin->h_bc_pinned;
        GL_HIP(hipMemcpy(w + kBcCtlBytes / 4u, sc.off, ((size_t)D + 2u) * 4u, hipMemcpyDeviceToHost));
    }
    const uint32_t *off = w + kBcCtlBytes / 4u;                   // off[L] .. off[L + 1]: level L's slice of the queue
    const uint32_t reached = n - off[1];
    if (pin->nnz == 0) {                                          // an empty graph: whoever has a level >= 2 is an orphan
        if (h_stats) {
            h_stats[0] = D;
            h_stats[1] = reached;
            h_stats[2] = D >= 2u ? n - off[2] : 0u;
        }
        return GL_OK;
    }
    BcSweepArgs a;
    a.level = d_level;
    a.ctl = sc.ctl;
    a.sigma = sigma;
    a.coef = sc.coef;
    a.bc = d_bc;
    a.scale = scale;
    a.n = n;
    a.cut_steps = shape_for(n).cut_steps;
    a.row_ptr = pin->d_csr_indptr;
    a.row_idx = pin->d_csr_indices;
    a.nz_base = pin->csr_nz_base;
    a.walk = 1u;
    for (uint32_t L = 2; L <= D; L++) {
        a.count = off[L + 1u] - off[L];
        if (a.count == 0u) continue;                              // (not a BFS result)
        a.queue = sc.queue + off[L];
        a.want = (float)(L - 1u);
        bc_sweep_kernel<true><<<shape_for(a.count).grid, 256, 0, s>>>(a);
    }
    GL_LAUNCH_CHECK();
    a.row_ptr = pout->d_csr_indptr;
    a.row_idx = pout->d_csr_indices;
    a.nz_base = pout->csr_nz_base;
    for (uint32_t L = D; L >= 2u; L--) {
        a.count = off[L + 1u] - off[L];
        if (a.count == 0u) continue;
        a.queue = sc.queue + off[L];
        a.want = (float)(L + 1u);
        a.walk = L < D ? 1u : 0u;
        bc_sweep_kernel<false><<<shape_for(a.count).grid, 256, 0, s>>>(a);
    }
    GL_LAUNCH_CHECK();
    if (h_stats) {
        GL_HIP(hipMemcpyAsync(w, sc.ctl, kBcCtlWords * 4u, hipMemcpyDeviceToHost, s));
        GL_HIP(hipStreamSynchronize(s));
        h_stats[0] = D;
        h_stats[1] = reached;
        h_stats[2] = w[kBcOrphans];
        h_stats[3] = w[kBcNonFinite];
    }
    return GL_OK;
}

}  // namespace gl

int gl_bc_accumulate(gl_spmv_plan plan_in, gl_spmv_plan plan_out, const float *d_level, double *d_bc, double scale, int accumulate,
                     double *d_sigma, uint32_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan_in != nullptr && plan_out != nullptr && d_level != nullptr && d_bc != nullptr);
    GL_ARG(d_sigma != d_bc);
    return gl::bc_accumulate(plan_in, plan_out, d_level, d_bc, scale, accumulate, d_sigma, h_stats, "gl_bc_accumulate");
}
