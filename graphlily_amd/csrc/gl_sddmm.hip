// SDDMM (gl_sddmm, graphlily_hip_sddmm.h): out[e] = a_e (x) (zero (+) sum_c X[r, c] (x) Y[j, c]) for every entry e = (r, j) of the
// plain CSR copy that a GL_PLAN_BOOLEAN plan keeps (gl_rows.h: rows_view), under the three semirings: two dense row-major blocks
// in, one f32 per stored entry out, in the numbering of gl_spmm's d_a_val.  The plan may be rectangular and a row shard; its rows
// need be neither sorted nor sets; an entry whose stored column is 0xffffffff (or not below num_cols) writes the literal 0.
//
// NOTHING IS SUMMED ACROSS A ROW'S ENTRIES: the sum runs over the k features and every entry is on its own.  So, unlike gl_spmm,
// no partial rows ever meet, a hub row is simply cut into pieces, and the cost is one contiguous k-float run of Y per entry
// against one run of X per row, which is held on chip.
//
// LANE LAYOUT (kept from the issue's design).  A wavefront is G groups of W lanes, G W = 64; a lane owns FOUR consecutive
// features of every tile of 4 W.  W is 1, 4, 16 or 64 for k <= 4, 16, 64 and above; for k > 256 a lane strides over the
// 256-feature tiles itself (T tiles in registers, T = 1, 2, 4 for k <= 256, 512, 1024): the reduction runs over the tiles, so
// the grid's second dimension is of no use.  A lane's partial sum runs tile by tile, feature by feature; the group's partial
// sums then meet by __shfl_xor at the distances 1, 2, ... W / 2.  That order depends on k alone, so every path and both load
// widths give the same bits.  A lane loads 16 bytes when the bases and leading dimensions allow it and its four features exist;
// otherwise it loads the features it has as dwords -- one load routine, decided per lane (sddmm_vec=0 forces the dwords).
//
// X STAYS ON CHIP.  Up to k = 1024 a lane keeps its slice of X's row in registers (at most 4 tiles x 4 floats = 16) for all the
// entries of the row or piece.  Above (kSddmmRegFeatures, a GUESS until measured) the WIDE kernel runs: a workgroup per row or
// piece stages the row in LDS once (up to 64 KiB = 16384 features; beyond that the lanes read it from memory through the same
// pointer) and its four wavefronts take the entries interleaved, a wavefront per entry.
//
// TWO PATHS by a row's entry count (lists from one counting pass, cached in the plan, keyed by the two knobs, not by k):
//   short   0 < count <= sddmm_cut   a group per row, G rows per wavefront step, four 16-byte Y loads per lane in flight (U
//                                    entries of T tiles, U T = 4) before the first product
//   piece   above                    the row is cut into pieces of sddmm_piece entries; the item is (row, piece), so a hub row
//                                    spreads over the device and nothing meets afterwards.  A wavefront per piece: per step it
//                                    loads 64 columns coalesced and hands them to the groups by __shfl -- group g takes the
//                                    entries = g (mod G) --; after the group reduction the G results of a step are handed
//                                    back by __shfl so that lane l stores entry base + l: one coalesced store (and one
//                                    coalesced load of a) per 64 entries
// sddmm_short=0 sends every row to the piece path.  Rows without entries are on no list.
//
// ARITHMETIC.  (+,x): products, sum, + zero and the scaling in f64 (the product of two f32 is exact in f64, so a fused
// multiply-add gives the bits of multiply, then add), one rounding to f32 at the store; no atomic.  (min,+): x + y in f32, the
// minimum, + a.  (||,&&): no value of A is read.  No matrix instruction: per row this is a (p x k)(k) matrix-vector product
// with a different GATHERED row of Y per output -- an MFMA tile would carry one useful column in sixteen -- and two of the
// three semirings are no multiply-add.  EXPERIMENTS.md Round 36 has the sweep the piece size was chosen from; the other defaults below are GUESSES.
#include "gl_rows.h"
#include "graphlily_hip_sddmm.h"

#include <algorithm>

namespace gl {

constexpr uint32_t kSddmmThreads = 256, kSddmmWaves = kSddmmThreads / 64u, kSddmmTile = 256;
constexpr long kSddmmCut = 32, kSddmmPiece = 256;      // the cut: a GUESS the sweep did not move; the piece: CHOSEN from the sweep
constexpr uint32_t kSddmmRegFeatures = 1024, kSddmmLdsFeatures = 16384;         // registers up to, LDS up to: GUESSES
constexpr uint32_t kSddmmPad = 0xffffffffu;

struct SddmmArgs {
    RowsView v;
    const float *a_val, *x, *y;
    float *out;
    const uint32_t *items;     // short: the rows' local numbers; piece: pairs {local row, piece}
    uint32_t nitems;
    uint64_t ldx, ldy;
    uint32_t k, piece;
    float zero;
    uint32_t vec;              // 16-byte loads are legal for a lane whose four features exist
    uint32_t lds;              // wide kernel: the row of X is staged in LDS
};

// the semirings over a lane's accumulator
template <int OP>
struct SddmmOp;
template <>
struct SddmmOp<GL_OP_MULADD> {
    typedef double acc_t;
    __device__ static acc_t init() { return 0.0; }
    __device__ static void step(acc_t &acc, float x, float y) { acc += (double)x * (double)y; }
    __device__ static acc_t merge(acc_t a, acc_t b) { return a + b; }
    __device__ static float finish(float zero, const float *a, acc_t acc) {
        const double s = (double)zero + acc;
        return (float)(a ? (double)*a * s : s);
    }
};
template <>
struct SddmmOp<GL_OP_ADDMIN> {
    typedef float acc_t;
    __device__ static acc_t init() { return __builtin_inff(); }
    __device__ static void step(acc_t &acc, float x, float y) {
        const float t = x + y;
        acc = t < acc ? t : acc;
    }
    __device__ static acc_t merge(acc_t a, acc_t b) { return b < a ? b : a; }
    __device__ static float finish(float zero, const float *a, acc_t acc) {
        const float m = acc < zero ? acc : zero;
        return a ? *a + m : m;
    }
};
template <>
struct SddmmOp<GL_OP_ANDOR> {
    typedef uint32_t acc_t;
    __device__ static acc_t init() { return 0u; }
    __device__ static void step(acc_t &acc, float x, float y) { acc |= x != 0.0f && y != 0.0f ? 1u : 0u; }
    __device__ static acc_t merge(acc_t a, acc_t b) { return a | b; }
    __device__ static float finish(float zero, const float *, acc_t acc) { return acc ? 1.0f : zero; }
};

struct SddmmQuad {
    float v[4];
};
// the ncol <= 4 floats at p: one 16-byte load, or the dword twin
__device__ __forceinline__ SddmmQuad sddmm_load4(const float *__restrict__ p, uint32_t ncol, bool vec) {
    SddmmQuad q;
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) q.v[u] = u < ncol ? p[u] : 0.0f;
    }
    return q;
}

// a lane's place in the feature tiles: its first feature of tile 0, how many of its four exist in each of its T tiles
template <int T>
struct SddmmLane {
    uint32_t c0, ncol[T];
    bool vec[T];
};
template <int W, int T>
__device__ __forceinline__ SddmmLane<T> sddmm_lane(const SddmmArgs &g, uint32_t lane) {
    SddmmLane<T> l;
    l.c0 = (lane % (uint32_t)W) * 4u;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const uint32_t c = l.c0 + (uint32_t)t * kSddmmTile;
        l.ncol[t] = c >= g.k ? 0u : g.k - c < 4u ? g.k - c : 4u;
        l.vec[t] = g.vec != 0u && l.ncol[t] == 4u;
    }
    return l;
}
template <int T>
__device__ __forceinline__ void sddmm_row(const float *__restrict__ p, const SddmmLane<T> &l, SddmmQuad (&q)[T]) {
#pragma unroll
    for (int t = 0; t < T; t++) q[t] = sddmm_load4(p + l.c0 + (uint32_t)t * kSddmmTile, l.ncol[t], l.vec[t]);
}

// U entries against the group's row of X: the Y loads first, all in flight, then each entry's sum in the one order -- the
// lane's tiles in turn, its features in turn, then the group's lanes by __shfl_xor at 1, 2, ... W / 2 (every lane of the group
// ends with the same bits).  Every lane of the wavefront comes here together; an entry with a pad column loads nothing.
template <int W, int T, int OP, int U>
__device__ __forceinline__ void sddmm_dots(const SddmmArgs &g, const SddmmLane<T> &l, const SddmmQuad (&xq)[T], const uint32_t (&col)[U],
                                           typename SddmmOp<OP>::acc_t (&res)[U]) {
    SddmmQuad yq[U][T];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int t = 0; t < T; t++) yq[u][t] = SddmmQuad{{0.0f, 0.0f, 0.0f, 0.0f}};
        if (col[u] < g.v.num_cols) sddmm_row<T>(g.y + (uint64_t)col[u] * g.ldy, l, yq[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        typename SddmmOp<OP>::acc_t acc = SddmmOp<OP>::init();
        if (col[u] < g.v.num_cols) {
#pragma unroll
            for (int t = 0; t < T; t++) {
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++)
                    if (q < l.ncol[t]) SddmmOp<OP>::step(acc, xq[t].v[q], yq[u][t].v[q]);
            }
        }
#pragma unroll
        for (int d = 1; d < W; d <<= 1) acc = SddmmOp<OP>::merge(acc, __shfl_xor(acc, d));
        res[u] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------- the short path
template <int W, int T, int OP>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_short_kernel(SddmmArgs g) {
    typedef typename SddmmOp<OP>::acc_t acc_t;
    constexpr uint32_t G = 64u / (uint32_t)W;
    constexpr int U = 4 / T;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = lane / (uint32_t)W;
    const SddmmLane<T> l = sddmm_lane<W, T>(g, lane);
    // (the loops' bounds are the wavefront's, not the group's: the shuffles want every lane)
    for (uint64_t it0 = ((uint64_t)blockIdx.x * kSddmmWaves + wave) * G; it0 < g.nitems; it0 += (uint64_t)gridDim.x * kSddmmWaves * G) {
        const bool have = it0 + grp < g.nitems;
        const uint32_t r = have ? g.items[it0 + grp] : 0u;
        const uint64_t b = have ? g.v.row_ptr[r] - g.v.nz_base : 0u, e = have ? g.v.row_ptr[r + 1u] - g.v.nz_base : 0u;
        SddmmQuad xq[T];
#pragma unroll
        for (int t = 0; t < T; t++) xq[t] = SddmmQuad{{0.0f, 0.0f, 0.0f, 0.0f}};
        if (have) sddmm_row<T>(g.x + ((uint64_t)g.v.row_begin + r) * g.ldx, l, xq);
        for (uint64_t j = b; __any(j < e); j += (uint32_t)U) {
            uint32_t col[U];
#pragma unroll
            for (uint32_t u = 0; u < (uint32_t)U; u++) col[u] = j + u < e ? g.v.row_idx[j + u] : kSddmmPad;
            acc_t res[U];
            sddmm_dots<W, T, OP, U>(g, l, xq, col, res);
            if (lane % (uint32_t)W == 0u) {
#pragma unroll
                for (uint32_t u = 0; u < (uint32_t)U; u++)
                    if (j + u < e) g.out[j + u] = col[u] < g.v.num_cols ? SddmmOp<OP>::finish(g.zero, g.a_val ? g.a_val + j + u : nullptr, res[u]) : 0.0f;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- the piece path
template <int W, int T, int OP>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_piece_kernel(SddmmArgs g) {
    typedef typename SddmmOp<OP>::acc_t acc_t;
    constexpr uint32_t G = 64u / (uint32_t)W;
    constexpr int U = 4 / T;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = lane / (uint32_t)W;
    const SddmmLane<T> l = sddmm_lane<W, T>(g, lane);
    for (uint64_t it = (uint64_t)blockIdx.x * kSddmmWaves + wave; it < g.nitems; it += (uint64_t)gridDim.x * kSddmmWaves) {
        const uint32_t r = g.items[2u * it], pc = g.items[2u * it + 1u];
        const uint64_t b = g.v.row_ptr[r] - g.v.nz_base + (uint64_t)pc * g.piece, row_e = g.v.row_ptr[r + 1u] - g.v.nz_base;
        const uint64_t e = row_e - b < g.piece ? row_e : b + g.piece;
        SddmmQuad xq[T];
        sddmm_row<T>(g.x + ((uint64_t)g.v.row_begin + r) * g.ldx, l, xq);
        for (uint64_t base = b; base < e; base += 64u) {
            const uint64_t j = base + lane;
            const uint32_t mycol = j < e ? g.v.row_idx[j] : kSddmmPad;
            const uint32_t n = e - base < 64u ? (uint32_t)(e - base) : 64u;
            acc_t mine = SddmmOp<OP>::init();
            for (uint32_t t0 = 0; t0 * G < n; t0 += (uint32_t)U) {
                uint32_t col[U];
#pragma unroll
                for (uint32_t u = 0; u < (uint32_t)U; u++) {
                    const uint32_t src = (t0 + u) * G + grp;
                    const uint32_t c = (uint32_t)__shfl((int)mycol, (int)(src & 63u));
                    col[u] = src < 64u ? c : kSddmmPad;
                }
                acc_t res[U];
                sddmm_dots<W, T, OP, U>(g, l, xq, col, res);
                // entry base + l was step l / G's, group l % G's: its result sits in that group's lanes
#pragma unroll
                for (uint32_t u = 0; u < (uint32_t)U; u++) {
                    const acc_t v = __shfl(res[u], (int)((lane % G) * (uint32_t)W));
                    if (lane / G == t0 + u) mine = v;
                }
            }
            if (j < e) g.out[j] = mycol < g.v.num_cols ? SddmmOp<OP>::finish(g.zero, g.a_val ? g.a_val + j : nullptr, mine) : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------- the wide kernel, k > 1024
// a workgroup per row (PIECES = false: the short list) or piece: X's row into LDS once, then a wavefront per entry, the four
// wavefronts interleaved; a lane strides over the tiles of 256 features in turn -- the order of the register kernels
template <int OP, bool PIECES>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_wide_kernel(SddmmArgs g) {
    typedef typename SddmmOp<OP>::acc_t acc_t;
    extern __shared__ __align__(16) float sddmm_xs[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t it = blockIdx.x; it < g.nitems; it += gridDim.x) {
        const uint32_t r = PIECES ? g.items[2u * it] : g.items[it];
        uint64_t b = g.v.row_ptr[r] - g.v.nz_base, e = g.v.row_ptr[r + 1u] - g.v.nz_base;
        if (PIECES) {
            b += (uint64_t)g.items[2u * it + 1u] * g.piece;
            e = e - b < g.piece ? e : b + g.piece;
        }
        const float *xr = g.x + ((uint64_t)g.v.row_begin + r) * g.ldx;
        if (g.lds) {
            __syncthreads();                                                  // the last item's row has been read
            for (uint32_t c = threadIdx.x; c < g.k; c += kSddmmThreads) sddmm_xs[c] = xr[c];
            __syncthreads();
            xr = sddmm_xs;
        }
        for (uint64_t j = b + wave; j < e; j += kSddmmWaves) {
            const uint32_t col = g.v.row_idx[j];
            if (col >= g.v.num_cols) {
                if (lane == 0u) g.out[j] = 0.0f;
                continue;
            }
            const float *yr = g.y + (uint64_t)col * g.ldy;
            acc_t acc = SddmmOp<OP>::init();
#pragma unroll 4
            for (uint32_t c = lane * 4u; c < g.k; c += kSddmmTile) {
                const uint32_t ncol = g.k - c < 4u ? g.k - c : 4u;
                const bool vec = g.vec != 0u && ncol == 4u;
                const SddmmQuad xq = sddmm_load4(xr + c, ncol, vec), yq = sddmm_load4(yr + c, ncol, vec);
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++)
                    if (q < ncol) SddmmOp<OP>::step(acc, xq.v[q], yq.v[q]);
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) acc = SddmmOp<OP>::merge(acc, __shfl_xor(acc, d));
            if (lane == 0u) g.out[j] = SddmmOp<OP>::finish(g.zero, g.a_val ? g.a_val + j : nullptr, acc);
        }
    }
}

// the one counting pass: a row of 0 < count <= cut entries into the short list (appended a wavefront's rows at a time), a longer
// one as its cdiv(count, piece) pieces into the piece list (the lists' order is of no consequence: no entry meets another)
__global__ __launch_bounds__(256) void sddmm_bin_kernel(const uint32_t *row_ptr, uint32_t rows, long long cut, uint32_t piece, uint32_t *counts,
                                                        uint32_t *short_list, uint32_t *piece_list) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < rows; i0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = i0 + threadIdx.x;
        const long long len = i < rows ? (long long)(row_ptr[i + 1u] - row_ptr[i]) : 0;
        const bool is_short = len > 0 && len <= cut;
        const uint64_t votes = __ballot(is_short);
        if (votes) {
            const int leader = __ffsll((unsigned long long)votes) - 1;
            uint32_t at = 0;
            if ((int)lane == leader) at = atomicAdd(counts, (uint32_t)__popcll(votes));
            at = (uint32_t)__shfl((int)at, leader);
            if (is_short) short_list[at + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = (uint32_t)i;
        }
        if (len > 0 && !is_short) {
            const uint32_t np = (uint32_t)((len + piece - 1) / piece), at = atomicAdd(counts + 1, np);
            for (uint32_t p = 0; p < np; p++) piece_list[2ull * (at + p)] = (uint32_t)i, piece_list[2ull * (at + p) + 1u] = p;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host
// the plan's scratch: 256 bytes of control words (the two counts), the short list of `rows` words, then (8-byte aligned) the
// piece list of nnz / piece + rows pairs -- a row of len > 0 entries has cdiv(len, piece) <= len / piece + 1 pieces
static size_t sddmm_piece_offset(uint32_t rows) { return 256 + (((size_t)std::max(rows, 1u) * 4u + 7u) & ~(size_t)7u); }

// the two lists for the knobs this call reads: built by the plan's first call and whenever the knobs have changed (one wait)
static int sddmm_prepare(gl_spmv_plan p, const char *who) {
    // A/B knobs (GRAPHLILY_DEBUG, read by every call): sddmm_cut = entries up to which a row is short, sddmm_piece = entries of a
    // piece (a multiple of 64: the piece path's stores stay aligned), sddmm_short = 0 closes the short path.  GUESSES.
    const long cut = debug_knob("sddmm_short", 1) != 0 ? std::max<long>(0, debug_knob("sddmm_cut", kSddmmCut)) : -1;
    const long piece = std::min<long>((std::max<long>(1, debug_knob("sddmm_piece", kSddmmPiece)) + 63) / 64 * 64, 1l << 30);
    if (p->d_sddmm_scratch && p->sddmm_cut == cut && p->sddmm_piece == piece) return GL_OK;
    hipStream_t s = ctx().stream;
    const uint32_t rows = p->row_end - p->row_begin;
    if (p->d_sddmm_scratch) {
        GL_HIP(hipStreamSynchronize(s));                                      // a call enqueued earlier may still read the old lists
        (void)hipFree(p->d_sddmm_scratch);
        p->d_sddmm_scratch = nullptr;
    }
    unsigned char *d = nullptr;
    const size_t off = sddmm_piece_offset(rows);
    int rc = plan_scratch(d, off + (p->nnz / (uint64_t)piece + rows) * 8u, who, "row and piece lists");
    if (rc != GL_OK) return rc;
    hipError_t e = hipMemsetAsync(d, 0, 256, s);
    if (e == hipSuccess) {
        sddmm_bin_kernel<<<rows_stream_grid(rows), 256, 0, s>>>(p->d_csr_indptr, rows, cut, (uint32_t)piece, reinterpret_cast<uint32_t *>(d),
                                                                reinterpret_cast<uint32_t *>(d + 256), reinterpret_cast<uint32_t *>(d + off));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(p->sddmm_items, d, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return set_error(GL_ERR_HIP, "%s: the row and piece lists: %s", who, hipGetErrorString(e));
    }
    p->d_sddmm_scratch = d;
    p->sddmm_cut = cut;
    p->sddmm_piece = piece;
    return GL_OK;
}

template <int W, int T, int OP>
static int sddmm_launch(gl_spmv_plan p, SddmmArgs g) {
    hipStream_t s = ctx().stream;
    constexpr unsigned G = 64u / (unsigned)W;
    const unsigned most = (unsigned)ctx().num_cus * 8u;
    if (p->sddmm_items[0]) {
        g.items = reinterpret_cast<const uint32_t *>(p->d_sddmm_scratch + 256);
        g.nitems = p->sddmm_items[0];
        sddmm_short_kernel<W, T, OP><<<std::min(cdiv(g.nitems, kSddmmWaves * G), most), kSddmmThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    if (p->sddmm_items[1]) {
        g.items = reinterpret_cast<const uint32_t *>(p->d_sddmm_scratch + sddmm_piece_offset(p->row_end - p->row_begin));
        g.nitems = p->sddmm_items[1];
        sddmm_piece_kernel<W, T, OP><<<std::min(cdiv(g.nitems, kSddmmWaves), most), kSddmmThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

template <int OP>
static int sddmm_launch_wide(gl_spmv_plan p, SddmmArgs g) {
    hipStream_t s = ctx().stream;
    const unsigned most = (unsigned)ctx().num_cus * 8u;
    g.lds = g.k <= kSddmmLdsFeatures ? 1u : 0u;
    const size_t lds_bytes = g.lds ? (size_t)g.k * 4u : 0u;
    if (p->sddmm_items[0]) {
        g.items = reinterpret_cast<const uint32_t *>(p->d_sddmm_scratch + 256);
        g.nitems = p->sddmm_items[0];
        sddmm_wide_kernel<OP, false><<<std::min(g.nitems, most), kSddmmThreads, lds_bytes, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    if (p->sddmm_items[1]) {
        g.items = reinterpret_cast<const uint32_t *>(p->d_sddmm_scratch + sddmm_piece_offset(p->row_end - p->row_begin));
        g.nitems = p->sddmm_items[1];
        sddmm_wide_kernel<OP, true><<<std::min(g.nitems, most), kSddmmThreads, lds_bytes, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

template <int OP>
static int sddmm_by_k(gl_spmv_plan p, const SddmmArgs &g) {
    const uint32_t k = g.k;
    return k <= 4u      ? sddmm_launch<1, 1, OP>(p, g)
           : k <= 16u   ? sddmm_launch<4, 1, OP>(p, g)
           : k <= 64u   ? sddmm_launch<16, 1, OP>(p, g)
           : k <= 256u  ? sddmm_launch<64, 1, OP>(p, g)
           : k <= 512u  ? sddmm_launch<64, 2, OP>(p, g)
           : k <= kSddmmRegFeatures ? sddmm_launch<64, 4, OP>(p, g)
                                    : sddmm_launch_wide<OP>(p, g);
}

static bool sddmm_overlap(const float *a, uint64_t a_floats, const float *b, uint64_t b_floats) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_floats && b_floats && a0 < b0 + 4u * b_floats && b0 < a0 + 4u * a_floats;
}
static uint64_t sddmm_extent(uint64_t rows, uint64_t ld, uint32_t k) { return rows ? (rows - 1u) * ld + k : 0u; }

static int sddmm(gl_spmv_plan p, const float *d_a_val, const float *d_x, uint64_t ldx, const float *d_y, uint64_t ldy, float *d_out, uint32_t k, int op,
                 float zero, uint64_t *h_stats, const char *who) {
    if (sddmm_overlap(d_out, p->nnz, d_x, sddmm_extent(p->num_rows, ldx, k)) || sddmm_overlap(d_out, p->nnz, d_y, sddmm_extent(p->num_cols, ldy, k)) ||
        sddmm_overlap(d_out, p->nnz, d_a_val, p->nnz))
        return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: d_out overlaps d_x, d_y or d_a_val", who);
    if (h_stats) h_stats[0] = h_stats[1] = 0, h_stats[2] = cdiv(k, kSddmmTile);
    if (p->nnz == 0) return GL_OK;                                            // (a plan without entries keeps no row copy)
    int rc = rows_require(p, 0u, who, "the plan");
    if (rc != GL_OK) return rc;
    if (p->nnz > 0xffffffffull)
        return set_error(GL_ERR_UNSUPPORTED, "%s: the plan: %llu entries do not fit 32-bit offsets", who, (unsigned long long)p->nnz);
    if ((rc = sddmm_prepare(p, who)) != GL_OK) return rc;
    SddmmArgs g = {};
    g.v = rows_view(p);
    g.a_val = op == GL_OP_ANDOR ? nullptr : d_a_val;
    g.x = d_x;
    g.y = d_y;
    g.out = d_out;
    g.ldx = ldx, g.ldy = ldy;
    g.k = k;
    g.piece = (uint32_t)p->sddmm_piece;
    g.zero = zero;
    const auto quads = [](const void *ptr, uint64_t ld) { return ((uintptr_t)ptr & 15u) == 0u && (ld & 3u) == 0u; };
    g.vec = debug_knob("sddmm_vec", 1) != 0 && quads(d_x, ldx) && quads(d_y, ldy) ? 1u : 0u;
    rc = op == GL_OP_MULADD ? sddmm_by_k<GL_OP_MULADD>(p, g) : op == GL_OP_ADDMIN ? sddmm_by_k<GL_OP_ADDMIN>(p, g) : sddmm_by_k<GL_OP_ANDOR>(p, g);
    if (rc != GL_OK || !h_stats) return rc;
    GL_HIP(hipStreamSynchronize(ctx().stream));
    h_stats[0] = p->sddmm_items[0], h_stats[1] = p->sddmm_items[1];
    return GL_OK;
}

}  // namespace gl

int gl_sddmm(gl_spmv_plan plan, const float *d_a_val, const float *d_x, uint64_t ldx, const float *d_y, uint64_t ldy, float *d_out, uint32_t k, int op,
             float zero, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_x != nullptr && d_y != nullptr);
    GL_ARG(d_out != nullptr || plan->nnz == 0);
    GL_ARG(k != 0u && ldx >= k && ldy >= k);
    GL_ARG(op == GL_OP_MULADD || op == GL_OP_ANDOR || op == GL_OP_ADDMIN);
    return gl::sddmm(plan, d_a_val, d_x, ldx, d_y, ldy, d_out, k, op, zero, h_stats, "gl_sddmm");
}
