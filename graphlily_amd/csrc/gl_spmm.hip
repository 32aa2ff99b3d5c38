// SpMM (gl_spmm, graphlily_hip_spmm.h): Y = A (+).(x) X for a dense, row-major block X of k vectors, under the three semirings,
// with an optional dense mask of Y's shape, over the plain CSR copy that a GL_PLAN_BOOLEAN plan keeps (gl_rows.h: rows_view).  The
// values travel apart from the plan, an f32 per entry of the row copy.  The plan may be rectangular and a row shard; its rows need
// be neither sorted nor sets; an entry whose stored column is 0xffffffff (or not below num_cols) is skipped under every semiring.
//
// ONE PASS OVER A SERVES ALL k COLUMNS: an entry (r, j) costs one 4-byte column, one 4-byte value and a CONTIGUOUS run of X's row
// j -- up to 1 KiB per wavefront -- where k SpMV runs gather k lone words.
//
// LANE LAYOUT.  A wavefront is G groups of W lanes, G W = 64; a lane owns FOUR consecutive columns (a float4 of X's row, four
// accumulators in registers), a group a column tile of 4 W floats.  W is 1, 4, 16 or 64 for k <= 4, 16, 64 and above; k > 256
// takes tiles of 256 columns on the grid's second dimension, each of which re-walks the row.  A lane loads 16 bytes per entry
// when the bases and leading dimensions allow it and its four columns exist; otherwise (unaligned bases, a leading dimension that
// is no multiple of 4, the ragged last tile, spmm_vec=0) it loads the columns it has as dwords -- one load routine, decided per lane.
//
// THREE PATHS, a row's by its entry count (the lists are cached in the plan: one counting pass, keyed by the cuts, not by k):
//   short       count <= spmm_cut    a group per row, G rows per wavefront step: the group's lanes read the row's entries four
//                                    at a time (the same address in every lane of the group) and keep four X loads in flight
//   wavefront   count <= spmm_wg     a wavefront per row: per step it loads 4 x 64 columns and values coalesced (lane l the
//                                    entries base + 64 u + l) and hands them to the groups by __shfl -- group g takes the entries
//                                    = g (mod G) --, four X loads per lane in flight before the first accumulate; the groups'
//                                    partial sums meet by __shfl_xor at distance W, 2 W, ... 32
//   workgroup   above                the four wavefronts of a workgroup take the 256-entry steps of ONE row interleaved; their
//                                    partial tiles (f64 under (+,x): 4 x 64 x 4 doubles = 8 KiB of LDS) are added in wavefront order
// spmm_short=0 sends the short rows to the wavefront path, spmm_wave=0 the wavefront rows to the workgroup path.
//
// ARITHMETIC.  (+,x): every product and the whole row sum in f64 (the product of two f32 is exact in f64), one rounding to f32
// at the store; no floating-point atomic anywhere; the order of a row's sum is fixed by the row, k and the path, so two calls
// give the same bits.  (min,+): a + x in f32, then the minimum.  (||,&&): no value is read; 1.0 where an entry meets an X != 0.
// No matrix instruction: the rows are unstructured CSR and two of the three semirings are no multiply-add.
// Every default below is a starting value, a GUESS until measured (EXPERIMENTS.md Round 35).
#include "gl_rows.h"
#include "graphlily_hip_spmm.h"

#include <algorithm>

namespace gl {

constexpr uint32_t kSpmmThreads = 256, kSpmmWaves = kSpmmThreads / 64u, kSpmmTileCols = 256;
constexpr long kSpmmCut = 32, kSpmmWg = 4096;   // GUESSES
constexpr uint32_t kSpmmPad = 0xffffffffu;

struct SpmmArgs {
    RowsView v;
    const float *a_val, *x, *mask;
    float *y;
    const uint32_t *items;     // the path's rows, local numbers
    uint32_t nitems;
    uint64_t ldx, ldy, ldm;
    uint32_t k, tiles;
    float zero;
    uint32_t vec;              // 16-byte loads and stores are legal for a lane whose four columns exist
    uint32_t keep_zero;        // masked: 1 keeps the elements whose mask == 0 (WriteToZero), 0 those whose mask != 0
};

// the semirings over a lane's accumulators
template <int OP>
struct SpmmOp;
template <>
struct SpmmOp<GL_OP_MULADD> {
    typedef double acc_t;
    __device__ static acc_t init() { return 0.0; }
    __device__ static void step(acc_t &acc, float a, float x) { acc += (double)a * (double)x; }
    __device__ static acc_t merge(acc_t a, acc_t b) { return a + b; }
    __device__ static float finish(float zero, acc_t acc) { return (float)((double)zero + acc); }
};
template <>
struct SpmmOp<GL_OP_ADDMIN> {
    typedef float acc_t;
    __device__ static acc_t init() { return __builtin_inff(); }
    __device__ static void step(acc_t &acc, float a, float x) {
        const float t = a + x;
        acc = t < acc ? t : acc;
    }
    __device__ static acc_t merge(acc_t a, acc_t b) { return b < a ? b : a; }
    __device__ static float finish(float zero, acc_t acc) { return acc < zero ? acc : zero; }
};
template <>
struct SpmmOp<GL_OP_ANDOR> {
    typedef uint32_t acc_t;
    __device__ static acc_t init() { return 0u; }
    __device__ static void step(acc_t &acc, float, float x) { acc |= x != 0.0f ? 1u : 0u; }
    __device__ static acc_t merge(acc_t a, acc_t b) { return a | b; }
    __device__ static float finish(float zero, acc_t acc) { return acc ? 1.0f : zero; }
};

struct SpmmQuad {
    float v[4];
};
// the ncol <= 4 floats at p: one 16-byte load, or the dword twin
__device__ __forceinline__ SpmmQuad spmm_load4(const float *__restrict__ p, uint32_t ncol, bool vec) {
    SpmmQuad q;
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) q.v[u] = u < ncol ? p[u] : 0.0f;
    }
    return q;
}

// a lane's place in the column tile: its first column, how many of its four exist, whether it moves 16 bytes at a time
struct SpmmCols {
    uint64_t c0;
    uint32_t ncol;
    bool vec;
};
template <int W>
__device__ __forceinline__ SpmmCols spmm_cols(const SpmmArgs &g, uint32_t tile, uint32_t lane) {
    SpmmCols c;
    c.c0 = (uint64_t)tile * kSpmmTileCols + (lane % (uint32_t)W) * 4u;
    c.ncol = c.c0 >= g.k ? 0u : g.k - c.c0 < 4u ? (uint32_t)(g.k - c.c0) : 4u;
    c.vec = g.vec != 0u && c.ncol == 4u;
    return c;
}

// Y[r, c0 .. c0 + ncol) = mask ? finish(zero, acc) : the literal 0
template <int OP, bool MASKED>
__device__ __forceinline__ void spmm_store(const SpmmArgs &g, uint64_t r, const SpmmCols &c, const typename SpmmOp<OP>::acc_t (&acc)[4]) {
    if (c.ncol == 0u) return;
    float out[4];
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = SpmmOp<OP>::finish(g.zero, acc[q]);
    if (MASKED) {
        const SpmmQuad m = spmm_load4(g.mask + r * g.ldm + c.c0, c.ncol, c.vec);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if ((m.v[q] == 0.0f) != (g.keep_zero != 0u)) out[q] = 0.0f;
    }
    float *y = g.y + r * g.ldy + c.c0;
    if (c.vec) {
        *reinterpret_cast<float4 *>(y) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++)
            if (q < c.ncol) y[q] = out[q];
    }
}

// four entries of one row into a lane's accumulators: the X loads first, all in flight, then the accumulates in entry order
template <int OP>
__device__ __forceinline__ void spmm_four(const SpmmArgs &g, const SpmmCols &c, const uint32_t (&col)[4], const float (&a)[4],
                                          typename SpmmOp<OP>::acc_t (&acc)[4]) {
    SpmmQuad xq[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        xq[u] = SpmmQuad{{0.0f, 0.0f, 0.0f, 0.0f}};
        if (col[u] < g.v.num_cols) xq[u] = spmm_load4(g.x + (uint64_t)col[u] * g.ldx + c.c0, c.ncol, c.vec);
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (col[u] < g.v.num_cols) {
#pragma unroll
            for (int q = 0; q < 4; q++) SpmmOp<OP>::step(acc[q], a[u], xq[u].v[q]);
        }
}

// ------------------------------------------------------------------------------------------------------------- the short path
template <int W, int OP, bool MASKED>
__global__ __launch_bounds__(kSpmmThreads) void spmm_short_kernel(SpmmArgs g) {
    typedef typename SpmmOp<OP>::acc_t acc_t;
    constexpr uint32_t G = 64u / (uint32_t)W;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = lane / (uint32_t)W;
    for (uint32_t tile = blockIdx.y; tile < g.tiles; tile += gridDim.y) {
        const SpmmCols c = spmm_cols<W>(g, tile, lane);
        for (uint64_t it = ((uint64_t)blockIdx.x * kSpmmWaves + wave) * G + grp; it < g.nitems; it += (uint64_t)gridDim.x * kSpmmWaves * G) {
            const uint32_t r = g.items[it];
            const uint64_t e = g.v.row_ptr[r + 1u] - g.v.nz_base;
            acc_t acc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = SpmmOp<OP>::init();
            for (uint64_t j = g.v.row_ptr[r] - g.v.nz_base; j < e; j += 4u) {
                uint32_t col[4];
                float a[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; u++) {
                    const bool in = j + u < e;
                    col[u] = in ? g.v.row_idx[j + u] : kSpmmPad;
                    a[u] = OP != GL_OP_ANDOR && in ? g.a_val[j + u] : 0.0f;
                }
                spmm_four<OP>(g, c, col, a, acc);
            }
            spmm_store<OP, MASKED>(g, (uint64_t)g.v.row_begin + r, c, acc);
        }
    }
}

// ------------------------------------------------------------------------------------------- the wavefront's walk over a row
// the 256-entry steps first, first + stride, ... of the entries [b, e): every lane of the wavefront takes every step (shuffles)
template <int W, int OP>
__device__ __forceinline__ void spmm_wave_walk(const SpmmArgs &g, const SpmmCols &c, uint64_t b, uint64_t e, uint32_t first, uint32_t stride,
                                               uint32_t lane, typename SpmmOp<OP>::acc_t (&acc)[4]) {
    constexpr uint32_t G = 64u / (uint32_t)W;
    const uint32_t grp = lane / (uint32_t)W;
    for (uint64_t base = b + 256ull * first; base < e; base += 256ull * stride) {
        uint32_t col[4];
        float a[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint64_t j = base + 64u * u + lane;
            col[u] = j < e ? g.v.row_idx[j] : kSpmmPad;
            a[u] = OP != GL_OP_ANDOR && j < e ? g.a_val[j] : 0.0f;
        }
        const uint32_t n0 = e - base < 64u ? (uint32_t)(e - base) : 64u;  // the entries of the step's first 64: the later ones are no more
        for (uint32_t t = 0; t * G < n0; t++) {
            const int src = (int)(t * G + grp);
            uint32_t cc[4];
            float aa[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cc[u] = (uint32_t)__shfl((int)col[u], src);
                aa[u] = __shfl(a[u], src);
            }
            spmm_four<OP>(g, c, cc, aa, acc);
        }
    }
    // the groups' partial sums: afterwards every lane holds its columns' sum over all groups, the same bits in each
#pragma unroll
    for (int d = W; d < 64; d <<= 1) {
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = SpmmOp<OP>::merge(acc[q], __shfl_xor(acc[q], d));
    }
}

template <int W, int OP, bool MASKED>
__global__ __launch_bounds__(kSpmmThreads) void spmm_wave_kernel(SpmmArgs g) {
    typedef typename SpmmOp<OP>::acc_t acc_t;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.y; tile < g.tiles; tile += gridDim.y) {
        const SpmmCols c = spmm_cols<W>(g, tile, lane);
        for (uint64_t it = (uint64_t)blockIdx.x * kSpmmWaves + wave; it < g.nitems; it += (uint64_t)gridDim.x * kSpmmWaves) {
            const uint32_t r = g.items[it];
            acc_t acc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = SpmmOp<OP>::init();
            spmm_wave_walk<W, OP>(g, c, g.v.row_ptr[r] - g.v.nz_base, g.v.row_ptr[r + 1u] - g.v.nz_base, 0u, 1u, lane, acc);
            if (lane < (uint32_t)W) spmm_store<OP, MASKED>(g, (uint64_t)g.v.row_begin + r, c, acc);
        }
    }
}

template <int W, int OP, bool MASKED>
__global__ __launch_bounds__(kSpmmThreads) void spmm_wg_kernel(SpmmArgs g) {
    typedef typename SpmmOp<OP>::acc_t acc_t;
    __shared__ acc_t part[kSpmmWaves * 64u * 4u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.y; tile < g.tiles; tile += gridDim.y) {
        const SpmmCols c = spmm_cols<W>(g, tile, lane);
        for (uint32_t it = blockIdx.x; it < g.nitems; it += gridDim.x) {
            const uint32_t r = g.items[it];
            acc_t acc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = SpmmOp<OP>::init();
            spmm_wave_walk<W, OP>(g, c, g.v.row_ptr[r] - g.v.nz_base, g.v.row_ptr[r + 1u] - g.v.nz_base, wave, kSpmmWaves, lane, acc);
            __syncthreads();                                                  // the last row's tiles have been read
#pragma unroll
            for (int q = 0; q < 4; q++) part[(wave * 64u + lane) * 4u + q] = acc[q];
            __syncthreads();
            if (wave == 0u && lane < (uint32_t)W) {
                for (uint32_t w = 1; w < kSpmmWaves; w++) {
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] = SpmmOp<OP>::merge(acc[q], part[(w * 64u + lane) * 4u + q]);
                }
                spmm_store<OP, MASKED>(g, (uint64_t)g.v.row_begin + r, c, acc);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the streaming passes
// a plan without entries: Y = mask ? fill : 0 over the plan's rows
__global__ __launch_bounds__(256) void spmm_fill_kernel(float *y, uint64_t ldy, const float *mask, uint64_t ldm, uint32_t keep_zero, uint32_t row_begin,
                                                        uint32_t rows, uint32_t k, float fill) {
    const uint64_t total = (uint64_t)rows * k;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = row_begin + i / k, c = i % k;
        const bool keep = !mask || (mask[r * ldm + c] == 0.0f) == (keep_zero != 0u);
        y[r * ldy + c] = keep ? fill : 0.0f;
    }
}

// the one counting pass: every row into the list of its path, appended a wavefront's rows at a time
__global__ __launch_bounds__(256) void spmm_bin_kernel(const uint32_t *row_ptr, uint32_t rows, long long cut, long long wg, uint32_t *counts,
                                                       uint32_t *list0, uint32_t *list1, uint32_t *list2) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < rows; i0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = i0 + threadIdx.x;
        int bin = -1;
        if (i < rows) {
            const long long len = row_ptr[i + 1u] - row_ptr[i];
            bin = len <= cut ? 0 : len <= wg ? 1 : 2;
        }
        for (int b = 0; b < 3; b++) {
            const uint64_t votes = __ballot(bin == b);
            if (!votes) continue;
            const int leader = __ffsll((unsigned long long)votes) - 1;
            uint32_t at = 0;
            if ((int)lane == leader) at = atomicAdd(counts + b, (uint32_t)__popcll(votes));
            at = (uint32_t)__shfl((int)at, leader);
            if (bin == b) (b == 0 ? list0 : b == 1 ? list1 : list2)[at + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = (uint32_t)i;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host
// the plan's scratch: 256 bytes of control words (the three counts), then three lists of `rows` words
static uint32_t *spmm_list(gl_spmv_plan p, int b) {
    return reinterpret_cast<uint32_t *>(p->d_spmm_scratch + 256) + (size_t)b * (p->row_end - p->row_begin);
}

// on the plan's first call (one synchronisation): the knobs and the three row lists
static int spmm_prepare(gl_spmv_plan p, const char *who) {
    if (p->d_spmm_scratch) return GL_OK;
    hipStream_t s = ctx().stream;
    const uint32_t rows = p->row_end - p->row_begin;
    // A/B knobs (GRAPHLILY_DEBUG, read by the plan's first call): spmm_cut = entries up to which a row is short, spmm_wg = entries
    // above which a workgroup takes it, spmm_short / spmm_wave = 0 close those paths, spmm_vec = 0 forces the dword twin.  GUESSES.
    const long cut = std::max<long>(0, debug_knob("spmm_cut", kSpmmCut)), wg = std::max(cut, debug_knob("spmm_wg", kSpmmWg));
    p->spmm_cut = debug_knob("spmm_short", 1) != 0 ? cut : -1;
    p->spmm_wg = debug_knob("spmm_wave", 1) != 0 ? wg : -1;
    p->spmm_vec = debug_knob("spmm_vec", 1) != 0;
    unsigned char *d = nullptr;
    int rc = plan_scratch(d, 256 + 3 * (size_t)std::max(rows, 1u) * 4u, who, "row lists");
    if (rc != GL_OK) return rc;
    uint32_t *lists = reinterpret_cast<uint32_t *>(d + 256);
    hipError_t e = hipMemsetAsync(d, 0, 256, s);
    if (e == hipSuccess) {
        spmm_bin_kernel<<<rows_stream_grid(rows), 256, 0, s>>>(p->d_csr_indptr, rows, p->spmm_cut, p->spmm_wg, reinterpret_cast<uint32_t *>(d), lists,
                                                               lists + rows, lists + 2 * (size_t)rows);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(p->spmm_rows, d, 12, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return set_error(GL_ERR_HIP, "%s: the row lists: %s", who, hipGetErrorString(e));
    }
    p->d_spmm_scratch = d;
    return GL_OK;
}

template <int W, int OP, bool MASKED>
static int spmm_launch(gl_spmv_plan p, SpmmArgs g) {
    hipStream_t s = ctx().stream;
    constexpr unsigned G = 64u / (unsigned)W;
    const unsigned most = (unsigned)ctx().num_cus * 8u, gy = std::min(g.tiles, 65535u);
    if (p->spmm_rows[0]) {
        g.items = spmm_list(p, 0);
        g.nitems = p->spmm_rows[0];
        spmm_short_kernel<W, OP, MASKED><<<dim3(std::min(cdiv(g.nitems, kSpmmWaves * G), most), gy), kSpmmThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    if (p->spmm_rows[1]) {
        g.items = spmm_list(p, 1);
        g.nitems = p->spmm_rows[1];
        spmm_wave_kernel<W, OP, MASKED><<<dim3(std::min(cdiv(g.nitems, kSpmmWaves), most), gy), kSpmmThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    if (p->spmm_rows[2]) {
        g.items = spmm_list(p, 2);
        g.nitems = p->spmm_rows[2];
        spmm_wg_kernel<W, OP, MASKED><<<dim3(std::min(g.nitems, most), gy), kSpmmThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

template <int W, int OP>
static int spmm_by_mask(gl_spmv_plan p, const SpmmArgs &g) {
    return g.mask ? spmm_launch<W, OP, true>(p, g) : spmm_launch<W, OP, false>(p, g);
}
template <int W>
static int spmm_by_op(gl_spmv_plan p, const SpmmArgs &g, int op) {
    return op == GL_OP_MULADD ? spmm_by_mask<W, GL_OP_MULADD>(p, g) : op == GL_OP_ADDMIN ? spmm_by_mask<W, GL_OP_ADDMIN>(p, g)
                                                                                          : spmm_by_mask<W, GL_OP_ANDOR>(p, g);
}

static bool spmm_overlap(const float *a, uint64_t a_floats, const float *b, uint64_t b_floats) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a_floats && b_floats && a0 < b0 + 4u * b_floats && b0 < a0 + 4u * a_floats;
}
static uint64_t spmm_extent(uint64_t rows, uint64_t ld, uint32_t k) { return rows ? (rows - 1u) * ld + k : 0u; }

static int spmm(gl_spmv_plan p, const float *d_a_val, const float *d_x, uint64_t ldx, const float *d_mask, uint64_t ldm, float *d_y, uint64_t ldy,
                uint32_t k, int op, float zero, int mask_type, uint64_t *h_stats, const char *who) {
    const uint64_t y_floats = spmm_extent(p->num_rows, ldy, k);
    if (spmm_overlap(d_y, y_floats, d_x, spmm_extent(p->num_cols, ldx, k)) || (d_mask && spmm_overlap(d_y, y_floats, d_mask, spmm_extent(p->num_rows, ldm, k))))
        return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: d_y overlaps d_x or d_mask", who);
    hipStream_t s = ctx().stream;
    const uint32_t rows = p->row_end - p->row_begin, tiles = cdiv(k, kSpmmTileCols);
    const uint32_t keep_zero = mask_type == GL_MASK_WRITETOZERO ? 1u : 0u;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = 0, h_stats[3] = tiles;
    if (p->nnz == 0) {
        // (a plan without entries keeps no row copy)
        const float fill = op == GL_OP_MULADD ? (float)((double)zero + 0.0) : zero;
        if (rows) {
            spmm_fill_kernel<<<std::max(1u, std::min<unsigned>(cdiv((uint64_t)rows * k, 256u), (unsigned)ctx().num_cus * 8u)), 256, 0, s>>>(
                d_y, ldy, d_mask, ldm, keep_zero, p->row_begin, rows, k, fill);
            GL_LAUNCH_CHECK();
        }
        if (h_stats) GL_HIP(hipStreamSynchronize(s));
        return GL_OK;
    }
    int rc = rows_require(p, 0u, who, "the plan");
    if (rc != GL_OK) return rc;
    if (p->nnz > 0xffffffffull)
        return set_error(GL_ERR_UNSUPPORTED, "%s: the plan: %llu entries do not fit 32-bit offsets", who, (unsigned long long)p->nnz);
    if ((rc = spmm_prepare(p, who)) != GL_OK) return rc;
    SpmmArgs g = {};
    g.v = rows_view(p);
    g.a_val = d_a_val;
    g.x = d_x;
    g.mask = d_mask;
    g.y = d_y;
    g.ldx = ldx, g.ldy = ldy, g.ldm = ldm;
    g.k = k;
    g.tiles = tiles;
    g.zero = zero;
    g.keep_zero = keep_zero;
    const auto quads = [](const void *ptr, uint64_t ld) { return ((uintptr_t)ptr & 15u) == 0u && (ld & 3u) == 0u; };
    g.vec = p->spmm_vec && quads(d_x, ldx) && quads(d_y, ldy) && (!d_mask || quads(d_mask, ldm)) ? 1u : 0u;
    rc = k <= 4u ? spmm_by_op<1>(p, g, op) : k <= 16u ? spmm_by_op<4>(p, g, op) : k <= 64u ? spmm_by_op<16>(p, g, op) : spmm_by_op<64>(p, g, op);
    if (rc != GL_OK || !h_stats) return rc;
    GL_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < 3; b++) h_stats[b] = p->spmm_rows[b];
    return GL_OK;
}

}  // namespace gl

int gl_spmm(gl_spmv_plan plan, const float *d_a_val, const float *d_x, uint64_t ldx, const float *d_mask, uint64_t ldm, float *d_y, uint64_t ldy,
            uint32_t k, int op, float zero, int mask_type, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_x != nullptr && d_y != nullptr);
    GL_ARG(k != 0u && ldx >= k && ldy >= k);
    GL_ARG(mask_type == GL_NOMASK || mask_type == GL_MASK_WRITETOZERO || mask_type == GL_MASK_WRITETOONE);
    GL_ARG(mask_type == GL_NOMASK || (d_mask != nullptr && ldm >= k));
    GL_ARG(op == GL_OP_MULADD || op == GL_OP_ANDOR || op == GL_OP_ADDMIN);
    GL_ARG(op == GL_OP_ANDOR || d_a_val != nullptr);
    return gl::spmm(plan, d_a_val, d_x, ldx, mask_type == GL_NOMASK ? nullptr : d_mask, ldm, d_y, ldy, k, op, zero, mask_type, h_stats, "gl_spmm");
}
