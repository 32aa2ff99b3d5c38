// SpMV over a semiring for MI355X (gfx950): y = mask( zero (+) A (x) x ).
//
// Replaces the FPGA path  SpMVModule::load_and_format_matrix -> csr2cpsr
// (module/spmv_module.h:281-370, io/data_formatter.h:456-534) and
// kernel_spmv (hw/kernel_spmv_impl.h:392-819).
//
// What the hardware dictates (measured on MI355X, scripts/ubench_*.hip):
//   * the packed 8-byte (index,value) stream reads at ~7 TB/s (45 clocks of a CU's vector-memory pipe per 512 B);
//   * a random 4-byte gather of x costs a whole cache line (~100 G/s from a 10 MB vector), but a gather whose
//     64 lanes read NEIGHBOURING columns costs ~20 clocks, from L1 and L2 alike -- and that cost ADDS to the
//     stream's: only fewer bytes per entry or fewer gather instructions (x values served from LDS) make
//     the loop faster; unrolling and LDS window staging were measured and do not (issuing the next slot's stream loads
//     under the current slot's accumulates does, a little, since the accumulates became straight-line code: spmv_phase);
//   * in the real stream a gather costs ~4 + 2.2 clocks per distinct 128-byte line it touches, and a row block's
//     sweep touches every line of x that holds one of its columns -- so the cold entries index a PACKED copy of x
//     (never-gathered columns dropped, rare ones clustered by degree class), refilled per run by a helper kernel;
//   * LDS atomics on 4/8-byte integers and on f64 run at full rate, ds_add_f32 at a third of it.
// This file holds the GENERAL layout (7-byte cold / 6.19-byte hot entries) and the PATTERN layout (3-byte cold entries, row-packed
// hot records of 7 entries in 16 bytes, for column-constant matrices), both served by spmv_rbcs_kernel<OP, MASK, stream layout, UC, UH>; the
// (||,&&)-only bit layout lives in gl_spmv_bool.hip.
// Hence the layout -- the CDNA4 counterpart of the FPGA's "dense-vector tile in URAM + output buffer
// in URAM" partitioning (kernel_spmv_impl.h:470-495), with the roles swapped:
//   row block   <= 15295 consecutive rows whose accumulators live in LDS for the whole sweep
//               (f64 for (+,x), so ds_add_f64; 32-bit ordered-int min for (min,+); plain store for (||,&&));
//   entries     of a row block are stored COLUMN-SORTED and DELTA-CODED (gl_spmv_plan.h): a 16-bit row slot, an
//               8-bit delta to the previous entry's gather index and the value -- 7 bytes (3 in the pattern
//               layout); 64 entries = one group with one base index, a lane's index = base + the prefix sum of
//               the deltas over the lanes (DPP), so a wavefront step is a coalesced read and its 64 gathers of
//               x fall into a handful of adjacent cache lines;
//   segments    a row block's stream is cut into S equal pieces ("units", one workgroup each) so that
//               about 256*k equally sized units exist (256 CUs); units are numbered segment-major so
//               concurrently running workgroups sweep the same column window of x (L2 resident).
//   hot columns the H highest-degree columns of the shard (on power-law graphs 8K columns hold a third of
//               the non-zeros) are cached per workgroup in an LDS table; their entries need no vector-memory
//               gather and, sorted by column, form RUNS: the hot stream is run-coded (gl_spmv_plan.h) -- a
//               16-bit row slot (+ the value) per entry, the column as one bit per entry and a base per
//               group, slots numbered per unit -- 6.19 bytes per entry instead of 8 (general layout; the pattern
//               layout's hot entries are ROW-PACKED since round 6: gl_spmv_plan.h).  The loop is bound by the CU's vector-memory pipe (45 clocks per 512 B of
//               stream + 4 + 2.2 clocks per line of a cold gather), so bytes per entry are what is left to
//               save; a wavefront processes UC cold and UH hot stream elements per iteration.
//   hub rows    a row that owns more than ~1/48 of its block's entries would make many lanes of every
//               wavefront step hit one LDS word; its entries are spread over 16 private slots (chosen
//               by the entry's position in its group, i.e. at format time) that are summed before the
//               epilogue.
// S == 1: the workgroup writes y for its rows directly, mask and semiring finish fused (the
// write_to_out_ddr epilogue, kernel_spmv_impl.h:339-389).  S > 1: every unit stores its tile to its
// segment's plane of a scratch buffer and spmv_combine_kernel folds the planes in segment order --
// deterministic, no atomics, 4*(2S+1) bytes per row.
#include "gl_spmv_plan.h"
#include "gl_tile.h"

namespace gl {

#if defined(GL_UNIT_CLOCKS)
__device__ unsigned long long g_unit_clocks[2 * 4096];   // {start, end} of every unit of the last spmv_rbcs_kernel launch (100 MHz)
#endif

struct SpmvArgs {
    const unsigned char *entries;   // delta-coded cold elements
    const uint32_t *bases;    // one base gather index per cold group
    const uint4 *units;       // 3 per unit: {first cold group, #cold groups, first row, #rows | direct << 31},
                              // {hub offset, #hub rows, #hot groups, segment}, {first hot element, present offset, #present, -}
    const uint32_t *hub_rows; // row_in_block of every hub row, per block
    const float *hot_x;       // x[hot_cols[k]], gathered once per run by the helper kernel
    uint32_t nhot;            // LDS table length: the longest present list, multiple of 64
    uint32_t tile_bytes;      // LDS bytes of the accumulator tile in front of the table (multiple of 16)
    const unsigned char *hot; // run-coded hot elements (gl_spmv_plan.h)
    const uint32_t *hot_hdr;  // per element: HG x {mask lo, mask hi}, HG x base
    const uint16_t *present;  // per unit: the slots of hot_x that occur in it, ascending
    const float *x;
    const float *mask;
    float *y;
    float zero;
    const float *xg;          // general plans: what the cold entries gather from (x, or the plan's packed copy of it)
    const float *z;           // pattern plans: colval (x) x (packed like xg), written by spmv_prescale_kernel
    const float *diag;        // pattern plans with diagonal exceptions: A[r][r] per local row, folded in by the epilogue
    const uint32_t *diag_has; // bit per local row: the row has a diagonal entry that differs from its column's value
    const uint32_t *run_flag;    // non-null: the launch is a no-op unless run_flag[0] != 0 (gl_spmspv_run's direction switch)
    float *partials;          // [segment][row - row_begin] per-unit tiles of split blocks (combined by spmv_combine_kernel)
    uint32_t prow;            // rows per segment plane
    uint32_t row_begin;
    uint32_t tickets;         // 1: wavefronts draw iterations from the LDS ticket; 0: static split (A/B builds)
    const uint32_t *self_hot_cols;   // non-null: no helper launch ran -- every workgroup gathers its (small) hot table from x itself
    // chained runs (gl_spmv_plan_chain): where y[row] goes in the NEXT run's packed vector / hot table (colmap: bit 31 = hot slot,
    // 0xffffffff = nowhere), times chain_colval[row] in pattern plans; null: not chained
    const uint32_t *chain_map = nullptr;
    const float *chain_colval = nullptr;
    float *chain_packed = nullptr, *chain_hot = nullptr;
};

// after the sweep: hub slots -> rows, then y (unsplit blocks) or this unit's plane (split blocks)
template <int OP, int MASK>
__device__ __forceinline__ void spmv_unit_epilogue(const SpmvArgs &a, typename Tile<OP>::T *tile, const uint4 d, const uint4 dh) {
    using TL = Tile<OP>;
    using T = typename TL::T;
    const uint32_t row0 = d.z, nrows = d.w & 0xffffu;
    const bool direct = (d.w >> 31) != 0u;
    const uint32_t hub_off = dh.x, nhub = dh.y;
    __syncthreads();
    if (nhub) {   // fold the private slots of every hub row back into its row
        if (threadIdx.x < nhub) {
            const uint32_t r = a.hub_rows[hub_off + threadIdx.x];
            T acc = tile[r];
#pragma unroll
            for (uint32_t k = 0; k < kHubSlots; k++) acc = TL::comb(acc, tile[nrows + kHubSlots * threadIdx.x + k]);
            tile[r] = acc;
        }
        __syncthreads();
    }

    if (direct) {
        for (uint32_t i = threadIdx.x; i < nrows; i += kThreads) {
            const uint32_t row = row0 + i;
            if (a.diag_has) {   // diagonal entries kept out of the stream (pattern plans, e.g. SSSP's zero self edges)
                const uint32_t lr = row - a.row_begin;
                if ((a.diag_has[lr >> 5] >> (lr & 31u)) & 1u)
                    tile[i] = TL::comb(tile[i], TL::lift(Semiring<OP>::mul(a.diag[lr], a.x[row])));
            }
            float out = TL::finish(a.zero, TL::get(tile, i));
            if (MASK != GL_NOMASK) {
                // masked-off rows are literal 0, and the mask is compared with 0 (spmv_module.h:518-530)
                if (!mask_allows_zero<MASK, OP>(a.mask[row])) out = 0.0f;
            }
            a.y[row] = out;
            if (MASK == GL_NOMASK && a.chain_map) {   // y is the next run's x: its packed form, as spmv_spread_x_kernel would leave it
                const uint32_t m = a.chain_map[row];
                if (m != 0xffffffffu) {
                    const float nx = a.chain_colval ? Semiring<OP>::mul(a.chain_colval[row], out) : out;
                    if (m >> 31) a.chain_hot[m & 0x7fffffffu] = nx;
                    else a.chain_packed[m] = nx;
                }
            }
        }
    } else {
        // split block: this unit's tile goes to its segment plane; spmv_combine_kernel folds the planes in
        // segment order (deterministic, no atomics) and applies zero / mask
        float *plane = a.partials + (size_t)dh.w * a.prow + (row0 - a.row_begin);
        for (uint32_t i = threadIdx.x; i < nrows; i += kThreads) plane[i] = TL::get(tile, i);
    }
}


// ---------------------------------------------------------------- stream layouts
// One kernel body serves both layouts; a layout says what one lane reads per ELEMENT (the groups a wavefront step loads,
// stored lane-interleaved: lane L holds entry L of each of the element's groups).  gl_spmv_plan.h describes both codings.
//   COLD stream, delta-coded: 16-bit slots, 8-bit deltas, the index from the group's base + a prefix sum over the lanes
//     WIDE   8 B of slots + 4 B of deltas + 16 B of values per lane   4 groups  (general layout, 7 B per entry)
//     QUAD   16 B of slots + 8 B of deltas per lane                   8 groups  (pattern layout, 3 B per entry)
//   HOT stream, run-coded: 16-bit slots, the table slot from the element's header
//     WIDE   8 B of slots + 16 B of values per lane                   4 groups  (6.19 B per entry)
//     QUAD   ROW-PACKED instead (round 6): 16 B per lane = one record, 7 table slots of one row + the row slot  (2.29 B per entry)
// Pattern plans (every column's stored values are equal) fold the value into z[c] = colval[c] (x) x[c] once per run and
// gather z instead of x.  (Round 5 retired the 8-byte-per-lane NARROW / PAIR streams of rounds 1-2, and the 32-bit
// { delta << 14 | slot } cold keys of rounds 1-4.)
//   WIDE_KEEP / QUAD_KEEP: the same streams read without the non-temporal hint (plans that fit the Infinity Cache)
enum { kLayWide = 1, kLayQuad = 3, kLayWideKeep = 4, kLayQuadKeep = 5 };

__device__ __forceinline__ uint32_t load_stream_nt4(const uint32_t *p) {
#ifdef GL_STREAM_PLAIN
    return *p;
#else
    return __builtin_nontemporal_load(p);
#endif
}

// inclusive prefix sum over the 64 lanes of BOTH 16-bit halves of v at once (the halves must not carry: 63 x 255 < 2^16):
// four row_shr steps scan the 16-lane rows, row_bcast:15 / :31 carry the row totals on -- six DPP adds, no LDS
__device__ __forceinline__ uint32_t wave_scan_pairs(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);    // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2 and 3
    return v;
}

// SDWA forms the compiler does not pick on its own (it extracts the 16-bit half with v_and / v_bfe and then shifts or adds with a
// VOP3 instruction: two instructions where one does): half H (0 low, 1 high) of w, shifted left / added to a scalar
template <int H>
__device__ __forceinline__ uint32_t half_shl(uint32_t w, uint32_t sh) {
    uint32_t r;
    if (H == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(sh), "v"(w));
    else asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(sh), "v"(w));
    return r;
}
template <int H>
__device__ __forceinline__ uint32_t half_add(uint32_t w, uint32_t scalar) {
    uint32_t r;
    if (H == 0) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(r) : "v"(w), "s"(scalar));
    else asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD" : "=v"(r) : "v"(w), "s"(scalar));
    return r;
}

template <int L>
struct Lay;

template <>
struct Lay<kLayWide> {
    static constexpr int G = (int)kColdGroupsGeneral;
    static constexpr bool kValues = true;
    static constexpr bool kHotRows = false;   // run-coded hot stream
    struct E {
        uint2 slots;
        uint32_t deltas;
        uint4 vals;
    };
    template <bool KEEP>
    __device__ static E load_cold(const unsigned char *cold, size_t e, uint32_t lane) {
        const unsigned char *p = cold + e * kColdElemBytesGeneral;
        E c;
        c.slots = KEEP ? load_stream_keep(reinterpret_cast<const uint2 *>(p) + lane) : load_stream_nt(reinterpret_cast<const uint2 *>(p) + lane);
        c.deltas = KEEP ? reinterpret_cast<const uint32_t *>(p + 512)[lane] : load_stream_nt4(reinterpret_cast<const uint32_t *>(p + 512) + lane);
        c.vals = KEEP ? load_stream_keep16(reinterpret_cast<const uint4 *>(p + 768) + lane) : load_stream_nt16(reinterpret_cast<const uint4 *>(p + 768) + lane);
        return c;
    }
    __device__ static E load(const unsigned char *cold, size_t e, uint32_t lane) { return load_cold<false>(cold, e, lane); }
    // offs[k] = BYTE offset (4 x gather index) of this lane's entry of group k, relative to the group's base: the deltas are scaled
    // by the masks that unpack them (63 x 255 x 4 < 2^16: still no carry between the halves), so that the gather needs no shift --
    // a 32-bit offset next to the vector's scalar base address
    // (pk[j]: two groups' prefix sums in one register -- group k sits in pk[k & 1], half k >> 1)
    __device__ static void offsets(const E &c, uint32_t (&pk)[G / 2]) {
        pk[0] = wave_scan_pairs((c.deltas << 2) & 0x03fc03fcu), pk[1] = wave_scan_pairs((c.deltas >> 6) & 0x03fc03fcu);
    }
    __device__ static uint32_t gather_off(const uint32_t (&pk)[G / 2], int k, uint32_t base4) {   // base4 + the lane's offset of group k
        return (k >> 1) ? half_add<1>(pk[k & 1], base4) : half_add<0>(pk[k & 1], base4);
    }
    __device__ static uint32_t slot_w(const E &c, int k) { return k < 2 ? c.slots.x : c.slots.y; }   // group k's slot: half k & 1 of this word
    __device__ static uint32_t slot(const E &c, int k) {
        const uint32_t w = k < 2 ? c.slots.x : c.slots.y;
        return (k & 1) ? w >> 16 : w & 0xffffu;
    }
    __device__ static float val(const E &c, int k) { return __uint_as_float(k == 0 ? c.vals.x : k == 1 ? c.vals.y : k == 2 ? c.vals.z : c.vals.w); }
    struct H {
        uint2 rows;
        uint4 vals;
    };
    static constexpr int HG = (int)kHotGroupsGeneral;
    __device__ static H load_hot(const unsigned char *hot, size_t e, uint32_t lane) {
        const unsigned char *p = hot + e * kHotElemBytesGeneral;
        H h;
        h.rows = load_stream_nt(reinterpret_cast<const uint2 *>(p) + lane);
        h.vals = load_stream_nt16(reinterpret_cast<const uint4 *>(p + 512) + lane);
        return h;
    }
    __device__ static uint32_t hot_slot_w(const H &h, int k) { return k < 2 ? h.rows.x : h.rows.y; }
    __device__ static uint32_t hot_slot(const H &h, int k) {
        const uint32_t w = k < 2 ? h.rows.x : h.rows.y;
        return (k & 1) ? w >> 16 : w & 0xffffu;
    }
    __device__ static float hot_val(const H &h, int k) { return __uint_as_float(k == 0 ? h.vals.x : k == 1 ? h.vals.y : k == 2 ? h.vals.z : h.vals.w); }
};

template <>
struct Lay<kLayQuad> {
    static constexpr int G = (int)kColdGroupsPattern;
    static constexpr bool kValues = false;
    struct E {
        uint4 slots;
        uint2 deltas;
    };
    template <bool KEEP>
    __device__ static E load_cold(const unsigned char *cold, size_t e, uint32_t lane) {
        const unsigned char *p = cold + e * kColdElemBytesPattern;
        E c;
        c.slots = KEEP ? load_stream_keep16(reinterpret_cast<const uint4 *>(p) + lane) : load_stream_nt16(reinterpret_cast<const uint4 *>(p) + lane);
        c.deltas = KEEP ? load_stream_keep(reinterpret_cast<const uint2 *>(p + 1024) + lane) : load_stream_nt(reinterpret_cast<const uint2 *>(p + 1024) + lane);
        return c;
    }
    __device__ static E load(const unsigned char *cold, size_t e, uint32_t lane) { return load_cold<false>(cold, e, lane); }
    // (byte offsets: see Lay<kLayWide>; group k sits in pk[2 (k >> 2) + (k & 1)], half (k >> 1) & 1)
    __device__ static void offsets(const E &c, uint32_t (&pk)[G / 2]) {
        pk[0] = wave_scan_pairs((c.deltas.x << 2) & 0x03fc03fcu), pk[1] = wave_scan_pairs((c.deltas.x >> 6) & 0x03fc03fcu);
        pk[2] = wave_scan_pairs((c.deltas.y << 2) & 0x03fc03fcu), pk[3] = wave_scan_pairs((c.deltas.y >> 6) & 0x03fc03fcu);
    }
    __device__ static uint32_t gather_off(const uint32_t (&pk)[G / 2], int k, uint32_t base4) {
        const uint32_t w = pk[2 * (k >> 2) + (k & 1)];
        return ((k >> 1) & 1) ? half_add<1>(w, base4) : half_add<0>(w, base4);
    }
    __device__ static uint32_t slot_w(const E &c, int k) { return (k >> 1) == 0 ? c.slots.x : (k >> 1) == 1 ? c.slots.y : (k >> 1) == 2 ? c.slots.z : c.slots.w; }
    __device__ static uint32_t slot(const E &c, int k) {
        const uint32_t w = (k >> 1) == 0 ? c.slots.x : (k >> 1) == 1 ? c.slots.y : (k >> 1) == 2 ? c.slots.z : c.slots.w;
        return (k & 1) ? w >> 16 : w & 0xffffu;
    }
    __device__ static float val(const E &, int) { return 0.0f; }
    // ROW-PACKED hot stream (gl_spmv_plan.h): a lane's 16 bytes are one record -- fields 0..6 the table slots of seven entries
    // of one row, field 7 the row's slot
    static constexpr bool kHotRows = true;
    struct H {
        uint4 rows;
    };
    static constexpr int HG = 1;   // (an element is 64 records; no groups, no headers)
    __device__ static H load_hot(const unsigned char *hot, size_t e, uint32_t lane) {
        H h;
        h.rows = load_stream_nt16(reinterpret_cast<const uint4 *>(hot + e * kHotElemBytesRows) + lane);
        return h;
    }
    __device__ static uint32_t hot_slot_w(const H &h, int k) { return (k >> 1) == 0 ? h.rows.x : (k >> 1) == 1 ? h.rows.y : (k >> 1) == 2 ? h.rows.z : h.rows.w; }
    __device__ static uint32_t hot_slot(const H &h, int k) {   // field k of the record
        const uint32_t w = (k >> 1) == 0 ? h.rows.x : (k >> 1) == 1 ? h.rows.y : (k >> 1) == 2 ? h.rows.z : h.rows.w;
        return (k & 1) ? w >> 16 : w & 0xffffu;
    }
    __device__ static float hot_val(const H &, int) { return 0.0f; }
};

template <>
struct Lay<kLayWideKeep> : Lay<kLayWide> {
    __device__ static E load(const unsigned char *cold, size_t e, uint32_t lane) { return load_cold<true>(cold, e, lane); }
    __device__ static H load_hot(const unsigned char *hot, size_t e, uint32_t lane) {
        const unsigned char *p = hot + e * kHotElemBytesGeneral;
        H h;
        h.rows = load_stream_keep(reinterpret_cast<const uint2 *>(p) + lane);
        h.vals = load_stream_keep16(reinterpret_cast<const uint4 *>(p + 512) + lane);
        return h;
    }
};
template <>
struct Lay<kLayQuadKeep> : Lay<kLayQuad> {
    __device__ static E load(const unsigned char *cold, size_t e, uint32_t lane) { return load_cold<true>(cold, e, lane); }
    __device__ static H load_hot(const unsigned char *hot, size_t e, uint32_t lane) {
        H h;
        h.rows = load_stream_keep16(reinterpret_cast<const uint4 *>(hot + e * kHotElemBytesRows) + lane);
        return h;
    }
};

// One slot's work: UC cold and UH hot stream elements (either may be 0), in three pieces so that the loop below can keep the
// NEXT slot's stream loads in flight while this slot gathers and accumulates.  Every load is unconditional -- indices clamp to
// the stream's last element and the plan pads its arrays by one element -- because conditional loads make the compiler
// serialise them with s_waitcnt vmcnt(0); out-of-range elements are dropped at the accumulate.
// accumulator `byte_off` bytes into the tile (byte_off = slot x sizeof(T), formed by ONE SDWA shift of the entry's 16-bit slot)
template <int OP>
constexpr uint32_t kTileShift = sizeof(typename Tile<OP>::T) == 8 ? 3u : 2u;
// (the tile starts at LDS address 0 -- the kernel has no static LDS and checks it once -- so the byte offset IS the LDS address:
//  formed from an integer the accumulate needs no base-address add either)
template <int OP>
__device__ __forceinline__ typename Tile<OP>::T *slot_ptr(typename Tile<OP>::T *, uint32_t byte_off) {
    typedef __attribute__((address_space(3))) typename Tile<OP>::T LdsT;
    return (typename Tile<OP>::T *)(LdsT *)(uintptr_t)byte_off;
}

struct StreamGeom {
    uint32_t g0, c0, nc, nc_last, h0, nh, nh_last;
};

template <int L, int UC, int UH>
struct SlotRegs {
    using LY = Lay<L>;
    typename LY::E ec[UC > 0 ? UC : 1];
    uint32_t bc[UC > 0 ? UC : 1][LY::G];                                       // the cold groups' bases: scalar registers
    typename LY::H eh[UH > 0 ? UH : 1];
    uint32_t hm[UH > 0 ? UH : 1][2 * LY::HG], hb[UH > 0 ? UH : 1][LY::HG];     // run masks and bases: scalar registers
    uint32_t ic, ih;                                                            // first cold / hot element of the slot
};

// 1. the slot's stream loads (vector: the elements; scalar: bases and headers)
template <int L, int UC, int UH>
__device__ __forceinline__ void slot_load(const SpmvArgs &a, const StreamGeom &sg, uint32_t lane, uint32_t ic, uint32_t ih, SlotRegs<L, UC, UH> &r) {
    using LY = Lay<L>;
    constexpr int G = LY::G, HG = LY::HG;
    r.ic = ic, r.ih = ih;
#pragma unroll
    for (int u = 0; u < UC; u++) {
        const uint32_t ei = min(ic + u * kWaves, sg.nc_last);
        r.ec[u] = LY::load(a.entries, (size_t)sg.c0 + ei, lane);
#pragma unroll
        for (int k = 0; k < G; k++)   // (byte offsets: gather indices < 2^30; shifted on the scalar unit)
            r.bc[u][k] = __builtin_amdgcn_readfirstlane(load_const(a.bases + sg.g0 + G * ei + k) << 2);
    }
#pragma unroll
    for (int u = 0; u < UH; u++) {
        const size_t e = (size_t)sg.h0 + min(ih + u * kWaves, sg.nh_last);
        r.eh[u] = LY::load_hot(a.hot, e, lane);
        if constexpr (!LY::kHotRows) {
            const uint32_t *hd = a.hot_hdr + e * (kHotHdrWordsPerGroup * HG);
#pragma unroll
            for (int k = 0; k < 2 * HG; k++) r.hm[u][k] = load_const(hd + k);
#pragma unroll
            for (int k = 0; k < HG; k++) r.hb[u][k] = load_const(hd + 2 * HG + k);
        }
    }
}

// 2. the cold entries' gathers: indices from the prefix sums of the deltas
template <int L, int UC, int UH>
__device__ __forceinline__ void slot_gather(const float *xsrc, const SlotRegs<L, UC, UH> &r, float (&xc)[UC > 0 ? UC : 1][Lay<L>::G]) {
    using LY = Lay<L>;
    constexpr int G = LY::G;
#pragma unroll
    for (int u = 0; u < UC; u++) {
        uint32_t pk[G / 2];
#ifdef GL_ABLATE_SCAN      // scratch A/B builds (scripts/build_variant.sh WORK <name> -DGL_ABLATE_...): what does each part of the step cost?
#pragma unroll
        for (int k = 0; k < G / 2; k++) pk[k] = 0u;
#else
        LY::offsets(r.ec[u], pk);            // the lanes' byte offsets relative to their groups' bases: prefix sums of the (scaled) deltas
#endif
#pragma unroll
        for (int k = 0; k < G; k++) {
            const uint32_t off = LY::gather_off(pk, k, r.bc[u][k]);   // one SDWA add: the group's half of the packed sums + its scalar base
#ifdef GL_ABLATE_GATHER
            xc[u][k] = __uint_as_float(off);
#else
            // (scalar base address + 32-bit byte offset: the load's saddr form, no 64-bit address arithmetic per lane)
            xc[u][k] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(xsrc) + off);
#endif
        }
    }
}

// 3. the accumulates.  Padding entries name one of the block's DUMMY slots (behind its last accumulator, one per lane: the
// formatters write them), so an element's accumulates are straight-line code -- no per-entry compare and branch, and the table
// look-ups of a hot element are all in flight before the first accumulate waits for one (an LDS round trip per entry was the hot
// path's critical path: s_waitcnt lgkmcnt counts in order).  Only whole elements past the end of the unit's stream (clamped
// loads) are skipped, by a wave-uniform branch.
template <int OP, int L, int UC, int UH>
__device__ __forceinline__ void slot_accumulate(typename Tile<OP>::T *tile, const float *hot_x, const StreamGeom &sg,
                                                const SlotRegs<L, UC, UH> &r, const float (&xc)[UC > 0 ? UC : 1][Lay<L>::G]) {
    using TL = Tile<OP>;
    using LY = Lay<L>;
    constexpr int G = LY::G, HG = LY::HG;
#pragma unroll
    for (int u = 0; u < UH; u++) {
        if constexpr (LY::kHotRows) {
            // one record per lane: seven look-ups (random 4-byte LDS reads, all in flight together), combined in registers, ONE
            // accumulate for the record's row -- 1/7 of the LDS atomics of an entry-per-lane stream (f64 atomic on random rows:
            // 24.6 LDS clocks per wavefront instruction, random read: 7.1)
            if (r.ih + u * kWaves < sg.nh) {
                float hv[kHotRecEntries];
#pragma unroll
                for (int k = 0; k < (int)kHotRecEntries; k++) hv[k] = hot_x[LY::hot_slot(r.eh[u], k)];
#ifdef GL_ABLATE_ACC
                asm volatile("" ::"v"(hv[0]), "v"(hv[1]), "v"(hv[2]), "v"(hv[3]), "v"(hv[4]), "v"(hv[5]), "v"(hv[6]), "v"(LY::hot_slot(r.eh[u], 7)));
#else
                typename TL::T acc = TL::lift(hv[0]);
#pragma unroll
                for (int k = 1; k < (int)kHotRecEntries; k++) acc = TL::comb(acc, TL::lift(hv[k]));
                TL::accl(slot_ptr<OP>(tile, half_shl<1>(r.eh[u].rows.w, kTileShift<OP>)), 0u, acc);   // (field 7: the row's slot)
#endif
            }
        } else if (r.ih + u * kWaves < sg.nh) {
            float hv[HG];
#pragma unroll
            for (int k = 0; k < HG; k++) {
                // the entry's table slot: the group's base + the runs that start in the lanes below (v_mbcnt on the scalar mask)
                const uint32_t ts = __builtin_amdgcn_mbcnt_hi(r.hm[u][2 * k + 1], __builtin_amdgcn_mbcnt_lo(r.hm[u][2 * k], r.hb[u][k]));
                hv[k] = hot_x[ts];
            }
#pragma unroll
            for (int k = 0; k < HG; k++) {
#ifdef GL_ABLATE_ACC
                asm volatile("" ::"v"(LY::hot_slot(r.eh[u], k)), "v"(LY::hot_val(r.eh[u], k)), "v"(hv[k]));
#else
                typename TL::T *at = slot_ptr<OP>(tile, (k & 1) ? half_shl<1>(LY::hot_slot_w(r.eh[u], k), kTileShift<OP>)
                                                                : half_shl<0>(LY::hot_slot_w(r.eh[u], k), kTileShift<OP>));
                if (LY::kValues) TL::acc(at, 0u, LY::hot_val(r.eh[u], k), hv[k]);
                else TL::accz(at, 0u, hv[k]);
#endif
            }
        }
    }
#pragma unroll
    for (int u = 0; u < UC; u++) {
        if (r.ic + u * kWaves < sg.nc) {
#pragma unroll
            for (int k = 0; k < G; k++) {
#ifdef GL_ABLATE_ACC
                asm volatile("" ::"v"(LY::slot(r.ec[u], k)), "v"(LY::val(r.ec[u], k)), "v"(xc[u][k]));
#else
                // the accumulator's address: the tile starts at LDS address 0, so it is the 16-bit slot shifted -- one SDWA shift
                typename TL::T *at = slot_ptr<OP>(tile, (k & 1) ? half_shl<1>(LY::slot_w(r.ec[u], k), kTileShift<OP>)
                                                                : half_shl<0>(LY::slot_w(r.ec[u], k), kTileShift<OP>));
                if (LY::kValues) TL::acc(at, 0u, LY::val(r.ec[u], k), xc[u][k]);
                else TL::accz(at, 0u, xc[u][k]);
#endif
            }
        }
    }
}

// The slots [it, n) of one phase (cold + hot elements, cold only, hot only), SOFTWARE-PIPELINED: while slot i's gathers and
// accumulates run, slot i + 1's stream loads are already in flight.  Round 5's ablation builds (profiles/r05_ablation.txt)
// showed a step's parts ADDING up -- pattern layout on orkut 0.208 ms, without gathers 0.177, without accumulates 0.170, without
// both 0.108 = the stream alone at 7.2 TB/s -- i.e. the 16 wavefronts of a CU did not overlap one another's phases: each
// wavefront had its stream loads in flight for a fraction of its iteration only.  Order per slot: gathers of slot i, the ticket
// and the (unconditional, clamped) loads of slot i + 1, then -- s_waitcnt vmcnt counts in order, the compiler leaves exactly the
// younger loads outstanding -- the accumulates of slot i.  The last slot of a phase prefetches one clamped slot for nothing.
// Same-box A/B (profiles/r05_ab_pipelined.txt): general layout orkut 0.278 -> 0.275 ms, products 0.185 -> 0.181, hollywood 0.136
// -> 0.133, the shuffled community stand-in 0.303 -> 0.285 -- it is bound by its HBM traffic (PMC: 6.05 TB/s), little was left to
// overlap.  The PATTERN layout loses (pokec 0.045 -> 0.049, ogbl-ppa 0.044 -> 0.046, the large graphs flat): two sets of its 24
// header registers per hot element do not fit the scalar register file (v_writelane spills), and its step is bound by LDS
// atomics + VALU + gathers rather than by stream latency -- so only the general layout is pipelined (PIPE).
template <int OP, int L, int UC, int UH>
__device__ __forceinline__ uint32_t spmv_phase(const SpmvArgs &a, typename Tile<OP>::T *tile, const float *hot_x, const float *xsrc,
                                               const StreamGeom &sg, uint32_t lane, uint32_t it, uint32_t n, uint32_t *next_slot) {
    if (it >= n) return it;
    auto cold_of = [](uint32_t i) { return i / kWaves * (kWaves * UC) + i % kWaves; };
    auto hot_of = [](uint32_t i) { return i / kWaves * (kWaves * UH) + i % kWaves; };
    constexpr bool PIPE = Lay<L>::kValues;   // (round 6, with the header-free row-packed hot stream: still +-1 %, pokec -9 %: profiles/r06_ab_patpipe.txt)
    if (!PIPE) {
        // one slot at a time: its loads, the next slot's ticket (drawn while they are in flight: at the end of the step it would
        // wait for the step's own accumulates -- LDS operations complete in order), gathers, accumulates
        while (it < n) {
            SlotRegs<L, UC, UH> r;
            slot_load<L, UC, UH>(a, sg, lane, cold_of(it), hot_of(it), r);
            uint32_t ticket = 0;
            if (a.tickets && lane == 0) ticket = __hip_atomic_fetch_add(next_slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            float xc[UC > 0 ? UC : 1][Lay<L>::G];
            slot_gather<L, UC, UH>(xsrc, r, xc);
            slot_accumulate<OP, L, UC, UH>(tile, hot_x, sg, r, xc);
            it = a.tickets ? __builtin_amdgcn_readfirstlane(ticket) : it + kWaves;
        }
        return it;
    }
    SlotRegs<L, UC, UH> cur;
    slot_load<L, UC, UH>(a, sg, lane, cold_of(it), hot_of(it), cur);
    while (true) {
        // the next slot's ticket (wavefronts draw slots from an LDS counter: with a static split the hardware's oldest-first issue
        // lets the low wavefronts finish ~10 % early), drawn first: it returns behind the previous slot's accumulates (LDS
        // operations complete in order) while this slot's prefix scans and gathers are issued
        uint32_t ticket = 0;
        if (a.tickets && lane == 0) ticket = __hip_atomic_fetch_add(next_slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        float xc[UC > 0 ? UC : 1][Lay<L>::G];
        slot_gather<L, UC, UH>(xsrc, cur, xc);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t nxt = a.tickets ? __builtin_amdgcn_readfirstlane(ticket) : it + kWaves;
        SlotRegs<L, UC, UH> nx;
        slot_load<L, UC, UH>(a, sg, lane, cold_of(nxt), hot_of(nxt), nx);
        __builtin_amdgcn_sched_barrier(0);
        slot_accumulate<OP, L, UC, UH>(tile, hot_x, sg, cur, xc);
        it = nxt;
        if (it >= n) break;
        cur = nx;
    }
    return it;
}

// One workgroup per unit.  UC cold and UH hot stream ELEMENTS (Lay<L>::G / HG groups each) per wavefront iteration;
// group counts per unit are multiples of G / HG.
template <int OP, int MASK, int L, int UC, int UH>
__global__ __launch_bounds__(kThreads) void spmv_rbcs_kernel(SpmvArgs a) {
    using TL = Tile<OP>;
    using T = typename TL::T;
    using LY = Lay<L>;
    constexpr int G = LY::G, HG = LY::HG;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    // the tile first: its base is a compile-time constant, so an accumulate's address is one shift of the 16-bit slot (+ the
    // instruction's immediate offset); the hot table behind it (a.tile_bytes: multiple of 16)
    T *tile = reinterpret_cast<T *>(__builtin_assume_aligned(lds_raw, 16));
    if ((uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char *)lds_raw) != 0u) __builtin_trap();   // (see slot_ptr)
    float *hot_x = reinterpret_cast<float *>(__builtin_assume_aligned(lds_raw + a.tile_bytes, 16));

    if (a.run_flag && *a.run_flag == 0u) return;
#if defined(GL_UNIT_CLOCKS)
    const unsigned long long unit_t0 = wall_clock64();
#endif
    const uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x);   // pinned to an SGPR: see clock_stamp
    const uint4 d = load_const(a.units + 3u * unit), dh = load_const(a.units + 3u * unit + 1u);   // scalar loads
    const uint4 dp = load_const(a.units + 3u * unit + 2u);
    const uint32_t g0 = d.x, ncold = d.y, nrows = d.w & 0xffffu;
    const uint32_t nhub = dh.y, nhotg = dh.z;
    const uint32_t nslots = nrows + kHubSlots * nhub;
    const uint32_t lane = threadIdx.x & 63u;
    // wave id as a scalar so that group indices, and with them the base-column loads, stay in SGPRs
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // ticket: the first kWaves iterations are taken by wave number.  The word lives BEHIND the table (no static LDS: the tile then
    // starts at LDS address 0 and an accumulate's address is the 16-bit slot shifted, one SDWA instruction)
    uint32_t &next_iter = *reinterpret_cast<uint32_t *>(lds_raw + a.tile_bytes + (size_t)a.nhot * 4u);
    if (threadIdx.x == 0) next_iter = kWaves;
    if (UH > 0 && LY::kHotRows) {
        // row-packed hot stream: the plan's whole table under its global slot numbers (one coalesced copy), and behind it the
        // slot that padding fields name: the semiring's identity
        for (uint32_t i = threadIdx.x; i < dp.z; i += kThreads) hot_x[i] = a.hot_x[i];
        if (threadIdx.x < 64u) hot_x[dp.z + threadIdx.x] = TL::zident();
    } else if (UH > 0) {   // the table: the values of the hot columns that occur in this unit, in the unit's slot order
        const uint16_t *pres = a.present + dp.y;
        if (a.self_hot_cols) {   // short streams: a helper launch in front would cost more than these few scattered reads
            for (uint32_t i = threadIdx.x; i < dp.z; i += kThreads) hot_x[i] = a.x[a.self_hot_cols[pres[i]]];
        } else {
            for (uint32_t i = threadIdx.x; i < dp.z; i += kThreads) hot_x[i] = a.hot_x[pres[i]];   // ascending, nearly dense: L2 hits
        }
    }
    for (uint32_t i = threadIdx.x; i < nslots + kPadSlots; i += kThreads) tile[i] = TL::ident();   // (+ the dummies that padding entries name)
    __syncthreads();

    // The stream is consumed in rounds of kWaves slots: slot w of round j takes cold elements j*kWaves*UC + w + u*kWaves
    // (u < UC) and the hot ones likewise, so the slots of a round read contiguous stream and sweep the same columns
    // (stream read + global gather for cold, stream read + LDS lookup for hot).  Wavefronts draw slot numbers from an LDS
    // ticket: with a static split the hardware's oldest-first issue lets the low wavefronts finish ~10 % early and the
    // CU idles its memory pipe while the rest catch up.  Rounds past the end of the shorter stream touch only the other.
    const float *xsrc = LY::kValues ? a.xg : a.z;
    StreamGeom sg;
    sg.g0 = g0;
    sg.c0 = g0 / G, sg.nc = ncold / G, sg.h0 = dp.x, sg.nh = nhotg / HG;   // (elements)
    sg.nc_last = max(sg.nc, 1u) - 1u, sg.nh_last = max(sg.nh, 1u) - 1u;
    const uint32_t rc = (sg.nc + kWaves * UC - 1) / (kWaves * UC), rh = UH > 0 ? (sg.nh + kWaves * UH - 1) / (kWaves * UH) : 0u;
    const uint32_t n_both = min(rc, rh) * kWaves, n_all = max(rc, rh) * kWaves;
    uint32_t it = wave;
    it = spmv_phase<OP, L, UC, UH>(a, tile, hot_x, xsrc, sg, lane, it, n_both, &next_iter);
    if (rc > rh) it = spmv_phase<OP, L, UC, 0>(a, tile, hot_x, xsrc, sg, lane, it, n_all, &next_iter);
    else if (UH > 0) it = spmv_phase<OP, L, 0, UH>(a, tile, hot_x, xsrc, sg, lane, it, n_all, &next_iter);
    spmv_unit_epilogue<OP, MASK>(a, tile, d, dh);
#if defined(GL_UNIT_CLOCKS)
    // scratch builds (scripts/unit_clocks.py): what every unit of the last launch took, start of the workgroup to its last store
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && unit < 4096u) {
        g_unit_clocks[2u * unit] = unit_t0;
        g_unit_clocks[2u * unit + 1u] = wall_clock64();
    }
#endif
}

// z[j] = colval (x) x of gathered column j (all columns, or the packed ones), four per thread, and the hot table from
// the same products.  zcolval, zcols and z hold a multiple of four elements (the plan pads them).
template <int OP>
__global__ __launch_bounds__(256) void spmv_prescale_kernel(const float *__restrict__ x, const uint32_t *__restrict__ zcols,
                                                            const float *__restrict__ zcolval, float *__restrict__ z, uint32_t nz,
                                                            uint32_t num_cols,
                                                            const uint32_t *__restrict__ hot_cols, const float *__restrict__ hot_colval,
                                                            float *__restrict__ hot_x, uint32_t nhot,
                                                            const uint32_t *__restrict__ run_flag) {
    if (run_flag && *run_flag == 0u) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (4u * i < nz) {
        const float4 v = reinterpret_cast<const float4 *>(zcolval)[i];
        float4 xv;
        if (zcols) {
            const uint4 c = reinterpret_cast<const uint4 *>(zcols)[i];
            xv = make_float4(x[c.x], x[c.y], x[c.z], x[c.w]);
        } else {   // identity: x itself may end before the padded group of four does
            const uint32_t c = 4u * i, last = num_cols - 1u;
            xv = make_float4(x[c], x[min(c + 1u, last)], x[min(c + 2u, last)], x[min(c + 3u, last)]);
        }
        reinterpret_cast<float4 *>(z)[i] = make_float4(Semiring<OP>::mul(v.x, xv.x), Semiring<OP>::mul(v.y, xv.y),
                                                       Semiring<OP>::mul(v.z, xv.z), Semiring<OP>::mul(v.w, xv.w));
    }
    if (i < nhot) hot_x[i] = Semiring<OP>::mul(hot_colval[i], x[hot_cols[i]]);
}

// the one scattered read of the hot columns per run (the workgroups then copy the compact table), and the packed copy
// of the gathered columns if the plan has one (four per thread; ccols and xc hold a multiple of four elements)
__global__ __launch_bounds__(256) void spmv_hot_gather_kernel(const float *__restrict__ x, const uint32_t *__restrict__ hot_cols,
                                                              float *__restrict__ hot_x, uint32_t nhot,
                                                              const uint32_t *__restrict__ ccols, float *__restrict__ xc, uint32_t ncompact,
                                                              const uint32_t *__restrict__ run_flag) {
    if (run_flag && *run_flag == 0u) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nhot) hot_x[i] = x[hot_cols[i]];
    // four groups of four per thread, every load of a stage issued before the first use: the kernel is a chain of two
    // dependent loads and a store, i.e. latency-bound unless several chains are in flight per thread
    if (ncompact == 0u) return;
    const uint32_t n4 = (ncompact + 3u) / 4u, base = blockIdx.x * 1024u + threadIdx.x;
    uint4 c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = reinterpret_cast<const uint4 *>(ccols)[min(base + k * 256u, n4 - 1u)];
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = make_float4(x[c[k].x], x[c[k].y], x[c[k].z], x[c[k].w]);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (base + k * 256u < n4) reinterpret_cast<float4 *>(xc)[base + k * 256u] = v[k];
}

// The same two vectors filled in ONE STREAMING PASS over x: colmap[c] says where column c's value goes (bit 31: hot slot,
// else index into the packed vector, 0xffffffff: nowhere).  The gathering kernels above read x once per degree class
// (every class is an ascending column list that touches nearly every line of x: 4 x 12 MB on the orkut stand-in, plus
// the 8 MB index list); this one reads x and the map once and lets the L2 assemble the packed lines from the scattered
// 4-byte stores (each class region is written in ascending order).  Used when a quarter or more of the columns are
// gathered.  Four columns per thread, 256 apart, so every load and store instruction of a wavefront is contiguous.
template <int OP, bool PATTERN>
__global__ __launch_bounds__(256) void spmv_spread_x_kernel(const float *__restrict__ x, const uint32_t *__restrict__ colmap,
                                                            const float *__restrict__ colval_bycol, float *__restrict__ packed,
                                                            float *__restrict__ hot_x, uint32_t num_cols,
                                                            const uint32_t *__restrict__ run_flag) {
    if (run_flag && *run_flag == 0u) return;
    const uint32_t cb = blockIdx.x * 1024u + threadIdx.x, last = num_cols - 1u;
    uint32_t m[4];
    float v[4], kv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {   // every load of the thread issued before the first store
        const uint32_t c = cb + 256u * k, cc = min(c, last);
        m[k] = c < num_cols ? colmap[cc] : 0xffffffffu;
        v[k] = x[cc];
        kv[k] = PATTERN ? colval_bycol[cc] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (m[k] == 0xffffffffu) continue;
        const float out = PATTERN ? Semiring<OP>::mul(kv[k], v[k]) : v[k];
        if (m[k] >> 31) hot_x[m[k] & 0x7fffffffu] = out;
        else packed[m[k]] = out;
    }
}

// y initialisation for the rows of blocks that are split into several units
template <int OP, int MASK>
__global__ __launch_bounds__(256) void spmv_init_kernel(uint32_t r0, uint32_t r1, const float *__restrict__ mask,
                                                        float *__restrict__ y, float zero) {
    for (uint32_t r = r0 + blockIdx.x * 256u + threadIdx.x; r < r1; r += gridDim.x * 256u) {
        float out = Tile<OP>::init(zero);
        if (MASK != GL_NOMASK) {
            if (!mask_allows_zero<MASK, OP>(mask[r])) out = 0.0f;
        }
        y[r] = out;
    }
}

// second pass of split plans: y[r] = mask( zero (+) plane_0[r] (+) ... (+) plane_{S-1}[r] ), one workgroup per
// 256 rows of a block; (+,x) sums the float planes in double
template <int OP, int MASK>
__global__ __launch_bounds__(256) void spmv_combine_kernel(const uint4 *__restrict__ blocks, const float *__restrict__ partials,
                                                           uint32_t prow, uint32_t row_begin, const float *__restrict__ mask,
                                                           float *__restrict__ y, float zero, const float *__restrict__ x,
                                                           const float *__restrict__ diag, const uint32_t *__restrict__ diag_has,
                                                           const uint32_t *__restrict__ run_flag) {
    if (run_flag && *run_flag == 0u) return;
    const uint4 b = blocks[blockIdx.y];   // {first row, #rows, #segments, -}
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < b.y; i += gridDim.x * 256u) {
        const uint32_t row = b.x + i;
        const float *p = partials + (row - row_begin);
        const uint32_t lr = row - row_begin;
        const bool has_diag = diag_has && ((diag_has[lr >> 5] >> (lr & 31u)) & 1u);
        float s;
        if (OP == GL_OP_MULADD) {
            double acc = 0.0;
            for (uint32_t k = 0; k < b.z; k++) acc += (double)p[(size_t)k * prow];
            if (has_diag) acc += (double)(diag[lr] * x[row]);
            s = (float)acc;
        } else {
            float acc = Semiring<OP>::ident(zero);
            for (uint32_t k = 0; k < b.z; k++) acc = Semiring<OP>::add(acc, p[(size_t)k * prow]);
            if (has_diag) acc = Semiring<OP>::add(acc, Semiring<OP>::mul(diag[lr], x[row]));
            s = acc;
        }
        float out = Tile<OP>::finish(zero, s);
        if (MASK != GL_NOMASK) {
            if (!mask_allows_zero<MASK, OP>(mask[row])) out = 0.0f;
        }
        y[row] = out;
    }
}

// ---------------------------------------------------------------- GL_PLAN_REFERENCE_ORDER
// SpMVModule::compute_reference_results (module/spmv_module.h:478-532) evaluated the way the reference writes it: one
// thread per row, the row's entries in CSR order, a float accumulator that starts at `zero`, a separately rounded float
// multiply and add per entry (no FMA: `#pragma clang fp contract(off)` -- HIP's __fmul_rn / __fadd_rn are plain `*` / `+`
// and contract under hipcc's default -ffp-contract=fast, found by the first run of the test), std::min's operand order.  The
// result is bit-equal to the reference loop BY CONSTRUCTION -- which is the point: the fast layouts differ from it only
// in the order (and, for (+,x), the width) of the accumulation, and a run on this layout shows that nothing else does.
template <int OP, int MASK>
__global__ __launch_bounds__(256) void spmv_reference_order_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                                   const float *__restrict__ data, const float *__restrict__ x,
                                                                   const float *__restrict__ mask, float *__restrict__ y, float zero,
                                                                   uint32_t row_begin, uint32_t rows) {
#pragma clang fp contract(off)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < rows; i += gridDim.x * 256u) {
        float acc = zero;
        const uint32_t e1 = indptr[i + 1u];
        for (uint32_t e = indptr[i]; e < e1; e++) {
            const float a = data[e], xv = x[indices[e]];
            if (OP == GL_OP_MULADD) {
                {
                    const float prod = a * xv;                                   // y[r] += data[i] * x[col]  (:495)
                    acc = acc + prod;
                }
            } else if (OP == GL_OP_ANDOR) {
                acc = (acc != 0.0f || (a != 0.0f && xv != 0.0f)) ? 1.0f : 0.0f;   // y[r] = y[r] || (data && x)  (:498)
            } else {
                const float t = a + xv;                                       // std::min(y[r], data + x) == (t < y) ? t : y  (:501)
                acc = (t < acc) ? t : acc;
            }
        }
        const uint32_t row = row_begin + i;
        if (MASK != GL_NOMASK) {
            if (!mask_allows_zero<MASK, OP>(mask[row])) acc = 0.0f;          // masked-off rows are literal 0 (:518-530)
        }
        y[row] = acc;
    }
}

template <int OP>
static int launch_reference_order(gl_spmv_plan p, const float *x, const float *mask, float *y, float zero, int mask_type, hipStream_t s) {
    const uint32_t rows = p->row_end - p->row_begin;
    if (!rows) return GL_OK;
    const unsigned grid = std::min<unsigned>(cdiv(rows, 256), (unsigned)ctx().num_cus * 16u);
    switch (mask_type) {
        case GL_NOMASK:
            spmv_reference_order_kernel<OP, GL_NOMASK><<<grid, 256, 0, s>>>(p->d_csr_indptr, p->d_csr_indices, p->d_csr_data, x, mask, y, zero, p->row_begin, rows);
            break;
        case GL_MASK_WRITETOZERO:
            spmv_reference_order_kernel<OP, GL_MASK_WRITETOZERO><<<grid, 256, 0, s>>>(p->d_csr_indptr, p->d_csr_indices, p->d_csr_data, x, mask, y, zero, p->row_begin, rows);
            break;
        case GL_MASK_WRITETOONE:
            spmv_reference_order_kernel<OP, GL_MASK_WRITETOONE><<<grid, 256, 0, s>>>(p->d_csr_indptr, p->d_csr_indices, p->d_csr_data, x, mask, y, zero, p->row_begin, rows);
            break;
        default: return set_error(GL_ERR_INVALID_ARG, "gl_spmv_run: invalid mask type %d", mask_type);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int spmv_run_reference_order(gl_spmv_plan p, const float *x, const float *mask, float *y, int op, float zero, int mask_type, hipStream_t s) {
    switch (op) {
        case GL_OP_MULADD: return launch_reference_order<GL_OP_MULADD>(p, x, mask, y, zero, mask_type, s);
        case GL_OP_ANDOR: return launch_reference_order<GL_OP_ANDOR>(p, x, mask, y, zero, mask_type, s);
        case GL_OP_ADDMIN: return launch_reference_order<GL_OP_ADDMIN>(p, x, mask, y, zero, mask_type, s);
        default: return set_error(GL_ERR_INVALID_ARG, "gl_spmv_run: invalid semiring op %d", op);
    }
}

}  // namespace gl

namespace gl {

template <int OP, int MASK, int L, int UC, int UH>
static int launch_variant(gl_spmv_plan p, const SpmvArgs &a, size_t lds, hipStream_t s) {
    static int attr_device = -1;  // per template instantiation; the opt-in is per device (gl_init may switch devices)
    if (attr_device != ctx().device) {
        GL_HIP(hipFuncSetAttribute((const void *)spmv_rbcs_kernel<OP, MASK, L, UC, UH>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        attr_device = ctx().device;
    }
    spmv_rbcs_kernel<OP, MASK, L, UC, UH><<<p->nunits, kThreads, lds, s>>>(a);
    return GL_OK;
}


template <int OP, int MASK>
static int launch_spmv(gl_spmv_plan p, const SpmvArgs &a_in, hipStream_t s) {
    SpmvArgs a = a_in;
    const uint32_t rows = p->row_end - p->row_begin;
    if (rows == 0) return GL_OK;
    if (p->nunits == 0) {   // no stored entries in this shard: y = mask(zero)
        unsigned grid = std::min<unsigned>(cdiv(rows, 256), (unsigned)ctx().num_cus * 8u);
        if (a.run_flag) return set_error(GL_ERR_UNSUPPORTED, "gl_spmv_run: a shard without stored entries cannot run under a launch predicate");
        spmv_init_kernel<OP, MASK><<<grid, 256, 0, s>>>(p->row_begin, p->row_end, a.mask, a.y, a.zero);
        GL_LAUNCH_CHECK();
        return GL_OK;
    }
    // chained runs (gl_spmv_plan_chain): the previous run's epilogue left THIS x in packed form in the buffers p->chain_sel names, and
    // this run's epilogue leaves y in the other pair
    const bool can_chain = p->chain_on && MASK == GL_NOMASK && OP < 3 && OP != GL_OP_ANDOR && !a.run_flag && p->d_colmap && p->d_packed_twin;
    bool x_ready = false;
    if (can_chain) {
        x_ready = p->chain_ptr == a.x && p->chain_op == OP;
        const int cur = x_ready ? p->chain_sel : 0;
        float *packed[2] = {p->pattern ? p->d_z : p->d_xc, p->d_packed_twin}, *hot[2] = {p->d_hot_x, p->d_hot_x_twin};
        a.hot_x = hot[cur];
        if (p->pattern) a.z = packed[cur];
        else a.xg = packed[cur];
        a.chain_map = p->d_colmap;
        a.chain_colval = p->pattern ? p->d_colval_bycol : nullptr;
        a.chain_packed = packed[cur ^ 1];
        a.chain_hot = hot[cur ^ 1];
        p->chain_ptr = a.y, p->chain_sel = cur ^ 1, p->chain_op = OP;
    } else {
        p->chain_ptr = nullptr;
    }
    float *packed_now = const_cast<float *>(p->pattern ? a.z : a.xg), *hot_now = const_cast<float *>(a.hot_x);
    if (p->self_hot || x_ready) {
        // no helper launch: the workgroups gather their hot table themselves, the cold entries index x directly -- or the previous
        // run of a chain has left this x packed
    } else if (p->d_colmap) {
        if (p->pattern)
            spmv_spread_x_kernel<OP, true><<<cdiv(p->num_cols, 1024), 256, 0, s>>>(a.x, p->d_colmap, p->d_colval_bycol, packed_now, hot_now,
                                                                                       p->num_cols, a.run_flag);
        else
            spmv_spread_x_kernel<OP, false><<<cdiv(p->num_cols, 1024), 256, 0, s>>>(a.x, p->d_colmap, nullptr, packed_now, hot_now,
                                                                                        p->num_cols, a.run_flag);
        GL_LAUNCH_CHECK();
    } else if (p->pattern) {
        const uint32_t nz = p->ncompact ? p->ncompact : p->num_cols;
        spmv_prescale_kernel<OP><<<cdiv(std::max(cdiv(nz, 4), p->nhot), 256), 256, 0, s>>>(a.x, p->ncompact ? p->d_ccols : nullptr, p->d_colval, p->d_z,
                                                                                         nz, p->num_cols, p->d_hot_cols, p->d_hot_colval, p->d_hot_x,
                                                                                         p->nhot, a.run_flag);
        GL_LAUNCH_CHECK();
    } else if (p->nhot || p->ncompact) {
        spmv_hot_gather_kernel<<<std::max(cdiv(p->ncompact, 4096), cdiv(p->nhot, 256)), 256, 0, s>>>(a.x, p->d_hot_cols, p->d_hot_x, p->nhot, p->d_ccols,
                                                                                                p->d_xc, p->ncompact, a.run_flag);
        GL_LAUNCH_CHECK();
    }
    const size_t tile_bytes = (((size_t)p->max_block_rows + kPadSlots) * sizeof(typename Tile<OP>::T) + 15u) & ~(size_t)15u;   // + the dummy slots
    const size_t lds = (size_t)p->nhot_lds * 4u + tile_bytes + 16u;   // (+ the ticket word behind the table)
    a.tile_bytes = (uint32_t)tile_bytes;
    if (lds > kLdsBudget)
        return set_error(GL_ERR_UNSUPPORTED, "gl_spmv_run: this plan was created with GL_PLAN_NO_MULADD "
                         "(hot-column table sized for 4-byte accumulators); (+,x) needs a plan without it");
    Profiler &pf = prof();
    const bool timed = prof_take(pf);
    if (timed) GL_HIP(hipEventRecord(pf.events[2 * pf.used], s));
    int rc;
    // float plans whose device arrays fit the Infinity Cache (256 MB) but not the L2s keep their stream cached between runs
    // (same-box: googleplus general 88 MB 50.5 -> 57.6 %, pokec pattern 155 MB 0.059 -> 0.047 ms, ogbl-ppa pattern 173 MB
    // 0.048 -> 0.046 ms; the 45 MB googleplus pattern plan lost 3 %: below 64 MB the hint stays)
    static const size_t keep_bytes = (size_t)224 << 20;
    static const size_t keep_min = (size_t)64 << 20;
    const bool keep = OP < 3 && p->device_bytes <= keep_bytes && p->device_bytes >= keep_min;
    // p->mix: cold / hot stream elements per wavefront iteration (an element: 4 groups in the general layout, 8 in the pattern one)
#define GL_SPMV_MIXES(O, LAY)                                                                \
    switch (p->mix) {                                                                         \
        case 0: rc = launch_variant<O, MASK, LAY, 2, 0>(p, a, lds, s); break;                 \
        case 3: rc = launch_variant<O, MASK, LAY, 1, 1>(p, a, lds, s); break;                 \
        default: rc = launch_variant<O, MASK, LAY, 2, 1>(p, a, lds, s); break;                \
    }
    constexpr int OPK = OP < 3 ? OP : 0;   // (the integer value types never take the keep variants: no instantiations for them)
    if (OP < 3 && keep && p->pattern) {
        GL_SPMV_MIXES(OPK, kLayQuadKeep)
    } else if (OP < 3 && keep) {
        GL_SPMV_MIXES(OPK, kLayWideKeep)
    } else if (p->pattern) {
        GL_SPMV_MIXES(OP, kLayQuad)
    } else {
        GL_SPMV_MIXES(OP, kLayWide)
    }
#undef GL_SPMV_MIXES
    if (rc != GL_OK) return rc;
    GL_LAUNCH_CHECK();
    if (timed) {
        GL_HIP(hipEventRecord(pf.events[2 * pf.used + 1], s));
        pf.used++;
    }
    if (p->segments > 1) {
        const dim3 grid(std::max<unsigned>(1u, std::min<unsigned>(cdiv(p->max_plain_rows, 256), 64u)), p->nblocks);
        spmv_combine_kernel<OP, MASK><<<grid, 256, 0, s>>>(p->d_blocks, p->d_partials, rows, p->row_begin, a.mask, a.y, a.zero, a.x,
                                                             a.diag, a.diag_has, a.run_flag);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

template <int OP>
static int dispatch_mask(int mask_type, gl_spmv_plan p, const SpmvArgs &a, hipStream_t s) {
    switch (mask_type) {
        case GL_NOMASK: return launch_spmv<OP, GL_NOMASK>(p, a, s);
        case GL_MASK_WRITETOZERO: return launch_spmv<OP, GL_MASK_WRITETOZERO>(p, a, s);
        case GL_MASK_WRITETOONE: return launch_spmv<OP, GL_MASK_WRITETOONE>(p, a, s);
        default: return set_error(GL_ERR_INVALID_ARG, "gl_spmv_run: invalid mask type %d", mask_type);
    }
}

// y initialisation for plans whose units fold into y (shared with gl_spmv_bool.hip)
template <int OP>
static int init_rows_mask(int mask_type, uint32_t r0, uint32_t r1, const float *mask, float *y, float zero, hipStream_t s) {
    if (r1 <= r0) return GL_OK;
    const unsigned grid = std::min<unsigned>(cdiv(r1 - r0, 256), (unsigned)ctx().num_cus * 8u);
    switch (mask_type) {
        case GL_NOMASK: spmv_init_kernel<OP, GL_NOMASK><<<grid, 256, 0, s>>>(r0, r1, mask, y, zero); break;
        case GL_MASK_WRITETOZERO: spmv_init_kernel<OP, GL_MASK_WRITETOZERO><<<grid, 256, 0, s>>>(r0, r1, mask, y, zero); break;
        case GL_MASK_WRITETOONE: spmv_init_kernel<OP, GL_MASK_WRITETOONE><<<grid, 256, 0, s>>>(r0, r1, mask, y, zero); break;
        default: return set_error(GL_ERR_INVALID_ARG, "invalid mask type %d", mask_type);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int spmv_init_rows(int op, int mask_type, uint32_t r0, uint32_t r1, const float *mask, float *y, float zero, hipStream_t s) {
    switch (op) {
        case GL_OP_MULADD: return init_rows_mask<GL_OP_MULADD>(mask_type, r0, r1, mask, y, zero, s);
        case GL_OP_ANDOR: return init_rows_mask<GL_OP_ANDOR>(mask_type, r0, r1, mask, y, zero, s);
        case GL_OP_ADDMIN: return init_rows_mask<GL_OP_ADDMIN>(mask_type, r0, r1, mask, y, zero, s);
        case kOpU32MulAdd: return init_rows_mask<kOpU32MulAdd>(mask_type, r0, r1, mask, y, zero, s);
        case kOpU32AndOr: return init_rows_mask<kOpU32AndOr>(mask_type, r0, r1, mask, y, zero, s);
        case kOpU32AddMin: return init_rows_mask<kOpU32AddMin>(mask_type, r0, r1, mask, y, zero, s);
        case kOpFixMulAdd: return init_rows_mask<kOpFixMulAdd>(mask_type, r0, r1, mask, y, zero, s);
        case kOpFixAndOr: return init_rows_mask<kOpFixAndOr>(mask_type, r0, r1, mask, y, zero, s);
        case kOpFixAddMin: return init_rows_mask<kOpFixAddMin>(mask_type, r0, r1, mask, y, zero, s);
        default: return set_error(GL_ERR_INVALID_ARG, "invalid semiring op %d", op);
    }
}

}  // namespace gl

extern "C" {

int gl_spmv_plan_bits_words(gl_spmv_plan p, uint64_t *words) {
    GL_ARG(p != nullptr && words != nullptr);
    *words = p->boolean ? (uint64_t)p->nphases * gl::kBoolPhaseWords : 0ull;
    return GL_OK;
}

int gl_pack_bits(const float *d_x, uint32_t n, uint32_t *d_bits) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(n == 0 || (d_x != nullptr && d_bits != nullptr));
    GL_ARG(((uintptr_t)d_bits & 7u) == 0);
    return gl::pack_bits(d_x, n, d_bits, gl::ctx().stream);
}

int gl_unpack_bits(const uint32_t *d_bits, uint32_t n, float *d_x) {
    GL_REQUIRE_INIT();
    GL_ARG(n == 0 || (d_x != nullptr && d_bits != nullptr));
    return gl::unpack_bits(d_bits, n, d_x, gl::ctx().stream);
}

int gl_bfs_bits_begin_from(uint32_t *d_ctl, uint32_t ctl_words, const float *d_x, uint32_t n, uint32_t *d_bits, uint32_t bits_words,
                           const float *d_distance, gl_spmv_plan rows) {
    GL_REQUIRE_INIT();
    GL_ARG(d_ctl != nullptr && d_x != nullptr && d_bits != nullptr && n > 0 && (uint64_t)bits_words * 32u >= n);
    GL_ARG(((uintptr_t)d_ctl & 7u) == 0 && ctl_words >= 18u && ctl_words <= 65536u);
    GL_ARG((bits_words & 3u) == 0 && ((uintptr_t)d_bits & 15u) == 0);
    return gl::bfs_bits_begin_from(d_ctl, ctl_words, d_x, n, d_bits, bits_words, gl::ctx().stream, d_distance, rows);
}

int gl_spmv_run_bits(gl_spmv_plan p, const uint32_t *d_bits, const float *d_mask, float *d_y, float zero, int mask_type) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr && d_y != nullptr && d_bits != nullptr);
    GL_ARG(mask_type == GL_NOMASK || d_mask != nullptr);
    GL_ARG(((uintptr_t)d_bits & 15u) == 0);
    if (!p->boolean)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_spmv_run_bits: the plan does not hold the GL_PLAN_BOOLEAN layout");
    return gl::bool_plan_run(p, nullptr, d_bits, d_mask, d_y, zero, mask_type, gl::ctx().stream);
}

int gl_bfs_pull_step(gl_spmv_plan p, const uint32_t *d_bits_in, uint32_t *d_bits_out, float *d_distance, float level) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr && d_bits_in != nullptr && d_bits_out != nullptr && d_distance != nullptr);
    GL_ARG(d_bits_in != d_bits_out);
    GL_ARG((((uintptr_t)d_bits_in | (uintptr_t)d_bits_out) & 15u) == 0);
    if (!p->boolean)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_bfs_pull_step: the plan does not hold the GL_PLAN_BOOLEAN layout");
    return gl::bool_plan_bfs_step(p, d_bits_in, d_bits_out, d_distance, level, gl::ctx().stream);
}

int gl_bfs_bits_pull_step(gl_spmv_plan p, gl_spmspv_plan csc, const uint32_t *d_bits_in, uint32_t *d_bits_out, float *d_distance,
                          float level, uint32_t *d_ctl, uint32_t slot, float threshold, int may_continue, float back_threshold) {
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr && csc != nullptr && d_bits_in != nullptr && d_bits_out != nullptr && d_distance != nullptr);
    GL_ARG(d_ctl != nullptr && slot >= 1u && ((uintptr_t)d_ctl & 7u) == 0);
    GL_ARG(d_bits_in != d_bits_out);
    GL_ARG((((uintptr_t)d_bits_in | (uintptr_t)d_bits_out) & 15u) == 0);
    if (!p->boolean)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_bfs_bits_pull_step: the plan does not hold the GL_PLAN_BOOLEAN layout");
    const bool deferred = (may_continue & GL_BFS_DEFERRED) != 0;
    const bool whole = p->row_begin == 0 && p->row_end == p->num_rows && gl::spmspv_plan_whole(csc, p->num_rows);
    if (!whole && !deferred)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_bfs_bits_pull_step: a row shard's frontier counts are partial -- pass GL_BFS_DEFERRED "
                             "in may_continue and take the slot's decisions with gl_bfs_bits_decide after the all-gather");
    gl::BfsPullSchedule sched;
    gl::BfsBitsCtl &c = sched.ctl;
    c.ctl = d_ctl;
    c.slot = slot;
    c.n = p->num_rows ? p->num_rows : 1u;
    c.may_continue = (uint32_t)may_continue & 3u;
    c.threshold = threshold;
    c.back_threshold = back_threshold;
    c.heavy = gl::spmspv_heavy_work(csc);
    c.nnz_rows = gl::spmspv_plan_nnz(csc);
    c.bu_limit = (p->d_csr_indptr && gl::spmspv_plan_bfs_rows(csc) == p) ? gl::spmspv_bottom_up_limit(csc) : 0ull;
    // the new frontier's column lengths decide the direction of the NEXT slot's push: of no use to a schedule that never pushes
    const bool only_pulls = threshold < 0.0f;   // BFS.pull: gl_bfs_bits_begin(first_pull_slot = 0)
    const bool may_push = (may_continue & 2) != 0 && !only_pulls && !deferred;
    sched.indptr = may_push ? gl::spmspv_plan_indptr(csc) : nullptr;
    sched.ncols = gl::spmspv_plan_num_cols(csc);
    sched.push_acc = gl::spmspv_plan_bfs_acc(csc);
    sched.deferred = deferred;
    return gl::bool_plan_bfs_step(p, d_bits_in, d_bits_out, d_distance, level, gl::ctx().stream, &sched);
}

int gl_spmv_run(gl_spmv_plan p, const float *d_x, const float *d_mask, float *d_y, int op, float zero,
                int mask_type) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr && d_y != nullptr);
    GL_ARG(d_x != nullptr || p->nnz == 0);
    GL_ARG(mask_type == GL_NOMASK || d_mask != nullptr);
    if (p->reference_order) return gl::spmv_run_reference_order(p, d_x, d_mask, d_y, op, zero, mask_type, gl::ctx().stream);
    if (p->boolean) {
        if (op != GL_OP_ANDOR)
            return gl::set_error(GL_ERR_UNSUPPORTED, "gl_spmv_run: this plan was created with GL_PLAN_BOOLEAN and "
                                 "holds the sparsity pattern only; semiring op %d needs a plan without it", op);
        return gl::bool_plan_run(p, d_x, nullptr, d_mask, d_y, zero, mask_type, gl::ctx().stream);
    }
    return gl::spmv_run_general(p, d_x, d_mask, d_y, op, zero, mask_type, nullptr);
}

int gl_spmv_plan_chain(gl_spmv_plan p, int on, int *active) {
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr);
    if (active) *active = 0;
    p->chain_ptr = nullptr;
    p->chain_on = false;
    if (!on) return GL_OK;
    // what a chained run needs: the streaming helper's column map (so y's packed form is one store per row), every block written by
    // its own workgroup (no split plan: their y comes from the combining kernel), the whole square matrix (row r IS column r of the
    // next x).  Anything else: the runs stay as they are -- the call is a hint, not a mode
    if (p->boolean || p->reference_order || !p->d_colmap || p->segments > 1 || p->row_begin != 0 || p->row_end != p->num_rows ||
        p->num_rows != p->num_cols || p->packed_len == 0)
        return GL_OK;
    if (!p->d_packed_twin) {
        hipError_t e = hipMalloc((void **)&p->d_packed_twin, p->packed_len * sizeof(float));
        if (e == hipSuccess) e = hipMemsetAsync(p->d_packed_twin, 0, p->packed_len * sizeof(float), gl::ctx().stream);
        if (e == hipSuccess && p->hot_x_len) {
            e = hipMalloc((void **)&p->d_hot_x_twin, p->hot_x_len * sizeof(float));
            if (e == hipSuccess) e = hipMemsetAsync(p->d_hot_x_twin, 0, p->hot_x_len * sizeof(float), gl::ctx().stream);   // padding slots stay 0
        }
        if (e != hipSuccess) {
            (void)hipFree(p->d_packed_twin);
            (void)hipFree(p->d_hot_x_twin);
            p->d_packed_twin = p->d_hot_x_twin = nullptr;
            return gl::set_error(GL_ERR_HIP, "gl_spmv_plan_chain: %s", hipGetErrorString(e));
        }
        p->device_bytes += (p->packed_len + p->hot_x_len) * sizeof(float);
    }
    p->chain_on = true;
    if (active) *active = 1;
    return GL_OK;
}

int gl_spmv_run_typed(gl_spmv_plan p, const void *d_x, const void *d_mask, void *d_y, int op, uint32_t zero_bits, int mask_type,
                      int val_type) {
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr && d_y != nullptr);
    GL_ARG(d_x != nullptr || p->nnz == 0);
    GL_ARG(mask_type == GL_NOMASK || d_mask != nullptr);
    GL_ARG(op == GL_OP_MULADD || op == GL_OP_ANDOR || op == GL_OP_ADDMIN);
    const float zero = __builtin_bit_cast(float, zero_bits);
    if (val_type == GL_VAL_FLOAT) return gl_spmv_run(p, (const float *)d_x, (const float *)d_mask, (float *)d_y, op, zero, mask_type);
    if (val_type != GL_VAL_UNSIGNED && val_type != GL_VAL_UFIXED_32_8)
        return gl::set_error(GL_ERR_INVALID_ARG, "gl_spmv_run_typed: unknown value type %d", val_type);
    if (p->boolean || p->reference_order)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_spmv_run_typed: GL_PLAN_BOOLEAN / GL_PLAN_REFERENCE_ORDER plans serve float only; create the plan without the flag");
    return gl::spmv_run_general(p, (const float *)d_x, (const float *)d_mask, (float *)d_y, op + 3 * val_type, zero, mask_type, nullptr);
}

}  // extern "C"

namespace gl {
// the general / pattern layouts; run_flag as in SpmvArgs
int spmv_run_general(gl_spmv_plan p, const float *d_x, const float *d_mask, float *d_y, int op, float zero, int mask_type,
                     const uint32_t *run_flag) {
    if (p->boolean || p->reference_order) return set_error(GL_ERR_UNSUPPORTED, "spmv_run_general: boolean / reference-order layout");
    if ((p->flags & (GL_PLAN_BOOLEAN | GL_PLAN_NO_MULADD)) && (op == GL_OP_MULADD || op == gl::kOpFixMulAdd) && p->nhot_lds &&
        (size_t)p->nhot_lds * 4u + ((size_t)p->max_block_rows + gl::kPadSlots) * sizeof(gl::Tile<GL_OP_MULADD>::T) > gl::kLdsBudget)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_spmv_run: this plan was created with GL_PLAN_NO_MULADD "
                             "(hot-column table sized for 4-byte accumulators); (+,x) needs a plan without it");
    gl::SpmvArgs a;
    a.entries = reinterpret_cast<const unsigned char *>(p->d_entries);
    a.bases = p->d_bases;
    a.units = p->d_units;
    a.hub_rows = p->d_hub_rows;
    a.hot_x = p->d_hot_x;
    a.nhot = p->nhot_lds;
    a.hot = p->d_hot;
    a.hot_hdr = p->d_hot_hdr;
    a.present = p->d_present;
    a.x = d_x;
    a.xg = p->ncompact ? p->d_xc : d_x;
    a.mask = d_mask;
    a.y = d_y;
    a.zero = zero;
    a.run_flag = run_flag;
    a.z = p->d_z;
    a.diag = p->d_diag;
    a.diag_has = p->d_diag_has;
    a.partials = p->d_partials;
    a.prow = p->row_end - p->row_begin;
    a.row_begin = p->row_begin;
    static const uint32_t tickets = 1u;
    a.tickets = tickets;
    a.self_hot_cols = p->self_hot ? p->d_hot_cols : nullptr;
    hipStream_t s = gl::ctx().stream;
    int rc;
    switch (op) {   // op + 3 * value type (gl_common.h)
        case GL_OP_MULADD: rc = gl::dispatch_mask<GL_OP_MULADD>(mask_type, p, a, s); break;
        case GL_OP_ANDOR: rc = gl::dispatch_mask<GL_OP_ANDOR>(mask_type, p, a, s); break;
        case GL_OP_ADDMIN: rc = gl::dispatch_mask<GL_OP_ADDMIN>(mask_type, p, a, s); break;
        case gl::kOpU32MulAdd: rc = gl::dispatch_mask<gl::kOpU32MulAdd>(mask_type, p, a, s); break;
        case gl::kOpU32AndOr: rc = gl::dispatch_mask<gl::kOpU32AndOr>(mask_type, p, a, s); break;
        case gl::kOpU32AddMin: rc = gl::dispatch_mask<gl::kOpU32AddMin>(mask_type, p, a, s); break;
        case gl::kOpFixMulAdd: rc = gl::dispatch_mask<gl::kOpFixMulAdd>(mask_type, p, a, s); break;
        case gl::kOpFixAndOr: rc = gl::dispatch_mask<gl::kOpFixAndOr>(mask_type, p, a, s); break;
        case gl::kOpFixAddMin: rc = gl::dispatch_mask<gl::kOpFixAddMin>(mask_type, p, a, s); break;
        default: rc = gl::set_error(GL_ERR_INVALID_ARG, "gl_spmv_run: invalid semiring op %d", op); break;
    }
    return rc;
}

}  // namespace gl

// gl_init loads this translation unit's code object up front (HIP defers that to the unit's first launch, which would put
// tens of milliseconds into somebody's timed call)
namespace gl {
int preload_spmv() {
    hipFuncAttributes attr;
    GL_HIP(hipFuncGetAttributes(&attr, (const void *)spmv_hot_gather_kernel));
    return GL_OK;
}
}  // namespace gl

#if defined(GL_UNIT_CLOCKS)
// scratch builds only: {start, end} wall_clock64() stamps of the units of the last main SpMV launch (2 x 4096 words)
extern "C" int gl_debug_unit_clocks(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(gl::g_unit_clocks), sizeof(gl::g_unit_clocks)) == hipSuccess ? 0 : 1;
}
#endif
