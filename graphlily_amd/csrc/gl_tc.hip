// Triangle counting (gl_tc_count): sorted-set intersections over the plain CSR copy that every GL_PLAN_BOOLEAN plan keeps
// (gl_spmv_plan.h: d_csr_indptr / d_csr_indices), on a square, whole-matrix plan whose rows are strictly ascending sets N(v).
//
//   total  = sum over v, over u in N(v), of |N(v) & N(u)|                                         (64 bits)
//   per[x] = number of triples (v, u, w), u in N(v), w in N(v) & N(u), in which x is v, u or w    (64 bits each, optional)
//
// A formula about sets: an acyclic orientation (io.triangle_orient) gives every triangle once, a full symmetric pattern six
// times, a diagonal entry simply takes part.  Integer adds commute, so the result is exact whatever the order.
//
// THE PLAN'S FIRST CALL has it established that the rows are such sets (gl_rows.h: kRowsSets), then reads the
// row offsets back once and bins the rows by length on the host (longest first inside a bin); bins and caps are cached in the plan.
//   short  1 .. tc_short entries (32)        a sub-wave GROUP of tc_group lanes (16) per row: 256 / G rows per workgroup
//   wave   .. tc_wave entries (1024)         a wavefront per row, four to a workgroup
//   wide   .. tc_lds entries (4096)          a wavefront per row, one to a workgroup (the LDS BUDGET: 16 KiB of N(v) per wavefront)
//   long   more                              a wavefront per CHUNK of 256 entries of the row; N(v) stays in global memory
// A launch asks for LDS by the bin's longest row, not by the cap.  Later calls only enqueue.
//
// THE KERNEL, one template for the four bins: the group copies N(v) into its slice of LDS (short, wave, wide), then walks the
// two-hop stream: for every u of N(v) -- read from the LDS copy, the same address in every lane: a broadcast -- N(u) is loaded in
// coalesced pieces of G entries and every lane looks its w up in N(v) by a branch-free binary search (ds_read_b32 at addresses
// that converge: the first probes of all lanes are the same word).  tc_search=1 turns a pair round when N(u) is more than eight
// times longer than N(v): the lanes then take the x of N(v) and search N(u) in global memory -- the shorter list in the longer.
// Hits are counted per lane in a register; a wavefront adds its sum to the total with ONE 64-bit atomic at the end.  With
// per-vertex counts (a template parameter: the total-only kernels carry none of this) a piece's hits are counted by a ballot,
// which every lane of the group sees: w is credited per hit, u once per (v, u), v once per row (per chunk in the long bin) --
// where N(v) is in LDS the credits of u and w go to a word next to their entry of N(v) (LDS atomics) and reach global memory
// once per row, one 64-bit add per entry that earned any; the long bin adds them to global memory directly.
// Groups share no LDS and meet at no barrier: a slice is written and read by lanes of ONE wavefront, whose LDS operations
// complete in order.  No spin-waits, no hand-offs between workgroups.
#include "gl_rows.h"

namespace gl {

constexpr uint32_t kTcChunk = 256;         // entries of a long row per work item
constexpr uint32_t kTcMaxShort = 256;      // ceilings of the caps (knobs): a wavefront's slice of 4096 entries is 16 KiB of LDS,
constexpr uint32_t kTcMaxLds = 4096;       // 32 KiB with the credit words

struct TcArgs {
    const uint32_t *row_ptr, *row_idx;
    const uint32_t *items;                 // short / wave: row numbers; long: pairs {row, first entry of the chunk}
    unsigned long long *total, *per;
    uint32_t nitems, cap;                  // cap: entries of a group's LDS slice (>= the longest row of the bin)
    uint32_t nz_base;                      // the row offsets count from the caller's entry list, row_idx starts at this entry
    uint32_t flip;                         // tc_search: N(u) longer than flip x N(v) is searched instead of walked (0: never)
};

// lanes of one wavefront have written the slice / are about to overwrite it: LDS operations of a wavefront complete in order,
// the fence keeps the compiler from moving them across
__device__ __forceinline__ void tc_slice_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int G, bool PER, bool LDS>
__global__ __launch_bounds__(256) void tc_count_kernel(TcArgs a) {
    extern __shared__ uint32_t tc_lds[];
    const uint32_t groups = blockDim.x / G;                       // per workgroup (256 threads; 64 in the wide bin)
    const uint32_t gl = threadIdx.x & (G - 1u), grp = threadIdx.x / G;
    const uint32_t gshift = (threadIdx.x & 63u) & ~(G - 1u);      // the group's first lane in its wavefront
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    // the group's slice: N(v), and with per-vertex counts one credit word per entry of N(v) behind it
    uint32_t *slice = tc_lds + (LDS ? grp * a.cap * (PER ? 2u : 1u) : 0u);
    uint32_t *credit = slice + a.cap;
    unsigned long long mine = 0;                                  // this lane's hits (PER: the group's, in its lane 0)
    for (uint32_t it = blockIdx.x * groups + grp; it < a.nitems; it += gridDim.x * groups) {
        uint32_t v, j0 = 0;
        if (LDS) {
            v = a.items[it];
        } else {
            v = a.items[2u * it];
            j0 = a.items[2u * it + 1u];
        }
        const uint32_t beg = a.row_ptr[v], len = a.row_ptr[v + 1u] - beg;
        const uint32_t *nv = a.row_idx + (beg - a.nz_base);
        uint32_t j1 = len;
        if (LDS) {
            tc_slice_sync();
            for (uint32_t i = gl; i < len; i += G) {              // len <= cap: the host binned by these very offsets
                slice[i] = nv[i];
                if (PER) credit[i] = 0u;
            }
            tc_slice_sync();
        } else {
            j1 = min(len, j0 + kTcChunk);
        }
        uint32_t row_hits = 0;
        for (uint32_t j = j0; j < j1; j++) {
            const uint32_t u = LDS ? slice[j] : nv[j];            // < num_rows: established by the plan's first call
            const uint32_t ub = a.row_ptr[u], lu = a.row_ptr[u + 1u] - ub;
            const uint32_t *nu = a.row_idx + (ub - a.nz_base);
            uint32_t pair_hits = 0;
            const bool flip = a.flip != 0u && lu > (uint64_t)a.flip * len;
            // walk N(u) and look every w up in N(v) -- or, flipped, the shorter list in the longer: every x of N(v) in N(u)
            const uint32_t steps = flip ? len : lu;
            for (uint32_t k = gl; k - gl < steps; k += G) {
                bool hit = false;
                uint32_t w = 0, at = k;                           // at: w's position in N(v)
                if (k < steps) {
                    if (flip) {
                        w = LDS ? slice[k] : nv[k];
                        hit = nu[rows_lower_bound(nu, lu, w)] == w;
                    } else {
                        w = nu[k];
                        at = LDS ? rows_lower_bound(slice, len, w) : rows_lower_bound(nv, len, w);
                        hit = (LDS ? slice[at] : nv[at]) == w;
                    }
                }
                if (PER) {
                    pair_hits += (uint32_t)__popcll((__ballot(hit) >> gshift) & gmask);
                    if (hit) {
                        if (LDS) atomicAdd(credit + at, 1u);
                        else atomicAdd(a.per + w, 1ull);
                    }
                } else {
                    mine += hit ? 1u : 0u;
                }
            }
            if (PER) {
                if (gl == 0u && pair_hits != 0u) {
                    if (LDS) atomicAdd(credit + j, pair_hits);
                    else atomicAdd(a.per + u, (unsigned long long)pair_hits);
                }
                row_hits += pair_hits;
            }
        }
        if (PER) {
            if (LDS) {
                // the row's credits: one global add per entry of N(v) that earned any
                tc_slice_sync();
                for (uint32_t i = gl; i < len; i += G) {
                    const uint32_t c = credit[i];
                    if (c != 0u) atomicAdd(a.per + slice[i], (unsigned long long)c);
                }
            }
            if (gl == 0u && row_hits != 0u) {
                atomicAdd(a.per + v, (unsigned long long)row_hits);
                mine += row_hits;
            }
        }
    }
    // the wavefront's sum: every lane is back here
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0u && mine != 0ull) atomicAdd(a.total, mine);
}

template <int G, bool LDS>
static void tc_launch(const TcArgs &a, bool per, unsigned threads, unsigned grid, hipStream_t s) {
    const size_t lds = LDS ? (size_t)(threads / G) * a.cap * (per ? 8u : 4u) : 0u;
    if (per) tc_count_kernel<G, true, LDS><<<grid, threads, lds, s>>>(a);
    else tc_count_kernel<G, false, LDS><<<grid, threads, lds, s>>>(a);
}

// the plan's bins, on first use (one synchronisation); a matrix without entries has none: tc_items stay 0, the call only
// zeroes its outputs
static int tc_prepare(gl_spmv_plan p, const char *who) {
    hipStream_t s = ctx().stream;
    const uint32_t rows = p->num_rows;
    if (p->nnz != 0 && !p->d_tc_scratch) {
        // A/B knobs (GRAPHLILY_DEBUG, read by the plan's first call): tc_short = longest row a sub-wave group takes, tc_wave =
        // longest row of the wave bin, tc_lds = longest row staged in LDS at all (the LDS budget: longer rows are searched in
        // global memory)
        const uint32_t cap_short = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("tc_short", 32), kTcMaxShort));
        // (four slices with their credit words within the 64 KiB a launch may ask for: 4 x 2048 x 8 B)
        const uint32_t cap_wave = (uint32_t)std::max<long>(cap_short, std::min<long>(debug_knob("tc_wave", 1024), kTcMaxLds / 2u));
        const uint32_t cap_lds = (uint32_t)std::max<long>(cap_wave, std::min<long>(debug_knob("tc_lds", kTcMaxLds), kTcMaxLds));
        std::vector<uint32_t> ip((size_t)rows + 1u, 0u);
        GL_HIP(hipStreamSynchronize(s));
        if (rows) GL_HIP(hipMemcpy(ip.data(), p->d_csr_indptr, ((size_t)rows + 1u) * 4u, hipMemcpyDeviceToHost));
        std::vector<uint32_t> bin[3], chunks;
        for (uint32_t v = 0; v < rows; v++) {
            const uint32_t len = ip[v + 1u] - ip[v];
            if (len == 0u) continue;
            if (len <= cap_lds) {
                bin[len <= cap_short ? 0 : len <= cap_wave ? 1 : 2].push_back(v);
            } else {
                for (uint32_t j = 0; j < len; j += kTcChunk) {
                    chunks.push_back(v);
                    chunks.push_back(j);
                }
            }
        }
        for (auto &b : bin)   // longest first: the grid-stride deals rows of like length to the groups of a wavefront
            std::stable_sort(b.begin(), b.end(), [&](uint32_t x, uint32_t y) { return ip[x + 1u] - ip[x] > ip[y + 1u] - ip[y]; });
        const size_t words = bin[0].size() + bin[1].size() + bin[2].size() + chunks.size();
        unsigned char *d = nullptr;
        const int rc = plan_scratch(d, std::max<size_t>(words, 4u) * 4u, who, "row bins");
        if (rc != GL_OK) return rc;
        uint32_t *w = reinterpret_cast<uint32_t *>(d);
        hipError_t e = hipSuccess;
        size_t at = 0;
        for (auto &b : bin) {
            if (e == hipSuccess && !b.empty()) e = hipMemcpy(w + at, b.data(), b.size() * 4u, hipMemcpyHostToDevice);
            at += b.size();
        }
        if (e == hipSuccess && !chunks.empty()) e = hipMemcpy(w + at, chunks.data(), chunks.size() * 4u, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            GL_HIP(e);
        }
        p->d_tc_scratch = d;
        p->tc_items[0] = (uint32_t)bin[0].size();
        p->tc_items[1] = (uint32_t)bin[1].size();
        p->tc_items[2] = (uint32_t)bin[2].size();
        p->tc_items[3] = (uint32_t)(chunks.size() / 2u);
        // a launch asks for the bin's LONGEST row, not for the cap (the bins are sorted longest first)
        for (int b = 0; b < 3; b++) p->tc_cap[b] = bin[b].empty() ? 0u : (ip[bin[b][0] + 1u] - ip[bin[b][0]] + 3u) & ~3u;
    }
    return GL_OK;
}

static int tc_count(gl_spmv_plan p, uint64_t *d_total, uint64_t *d_per_vertex, const char *who) {
    int rc = rows_require(p, kRowsSets, who, "the plan", "io.triangle_orient");
    if (rc == GL_OK) rc = tc_prepare(p, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    GL_HIP(hipMemsetAsync(d_total, 0, 8, s));
    if (d_per_vertex && p->num_rows) GL_HIP(hipMemsetAsync(d_per_vertex, 0, 8u * (size_t)p->num_rows, s));
    // A/B knobs (GRAPHLILY_DEBUG, read per call): tc_group = lanes per short row (8, 16, 32 or 64), tc_search = 1 searches the
    // shorter list in the longer (a pair is turned round when N(u) is more than tc_flip = 8 times longer than N(v)),
    // tc_grid = workgroups per compute unit
    const long group = debug_knob("tc_group", 16);
    const unsigned per_cu = (unsigned)std::max<long>(1, std::min<long>(debug_knob("tc_grid", 32), 1024));
    const bool per = d_per_vertex != nullptr;
    TcArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.nz_base = p->csr_nz_base;
    a.total = reinterpret_cast<unsigned long long *>(d_total);
    a.per = reinterpret_cast<unsigned long long *>(d_per_vertex);
    a.flip = debug_knob("tc_search", 0) != 0 ? (uint32_t)std::max<long>(1, std::min<long>(debug_knob("tc_flip", 8), 1l << 20)) : 0u;
    const uint32_t *items = reinterpret_cast<const uint32_t *>(p->d_tc_scratch);
    auto grid_for = [&](uint32_t nitems, uint32_t groups) {
        return std::max(1u, std::min<unsigned>(cdiv(nitems, groups), (unsigned)ctx().num_cus * per_cu));
    };
    if (p->tc_items[0]) {
        a.items = items;
        a.nitems = p->tc_items[0];
        a.cap = p->tc_cap[0];
        switch (group) {
            case 8: tc_launch<8, true>(a, per, 256, grid_for(a.nitems, 32u), s); break;
            case 32: tc_launch<32, true>(a, per, 256, grid_for(a.nitems, 8u), s); break;
            case 64: tc_launch<64, true>(a, per, 256, grid_for(a.nitems, 4u), s); break;
            default: tc_launch<16, true>(a, per, 256, grid_for(a.nitems, 16u), s); break;
        }
        GL_LAUNCH_CHECK();
    }
    if (p->tc_items[1]) {
        a.items = items + p->tc_items[0];
        a.nitems = p->tc_items[1];
        a.cap = p->tc_cap[1];
        tc_launch<64, true>(a, per, 256, grid_for(a.nitems, 4u), s);
        GL_LAUNCH_CHECK();
    }
    if (p->tc_items[2]) {
        // the wide bin: one wavefront per workgroup, so that a slice of kTcMaxLds entries (16 KiB, 32 with the credits) stays
        // within the 64 KiB a launch may ask for and several workgroups share a compute unit
        a.items = items + p->tc_items[0] + p->tc_items[1];
        a.nitems = p->tc_items[2];
        a.cap = p->tc_cap[2];
        tc_launch<64, true>(a, per, 64, grid_for(a.nitems, 1u), s);
        GL_LAUNCH_CHECK();
    }
    if (p->tc_items[3]) {
        a.items = items + p->tc_items[0] + p->tc_items[1] + p->tc_items[2];
        a.nitems = p->tc_items[3];
        a.cap = 0;
        tc_launch<64, false>(a, per, 256, grid_for(a.nitems, 4u), s);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

}  // namespace gl

int gl_tc_count(gl_spmv_plan plan, uint64_t *d_total, uint64_t *d_per_vertex) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_total != nullptr);
    return gl::tc_count(plan, d_total, d_per_vertex, "gl_tc_count");
}
