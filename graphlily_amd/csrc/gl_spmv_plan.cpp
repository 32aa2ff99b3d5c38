// Host planning of the SpMV layouts (gl_spmv_plan.h): the row-block / segment planner and plan creation, destruction,
// description and export.  The kernels the plans feed live in gl_spmv.hip (general / pattern) and gl_spmv_bool.hip ((||,&&)).
#include "gl_spmv_plan.h"

#include <climits>
#include <memory>

namespace gl {

// ------------------------------------------------------------------------------------- planner
// matrix-stream rate (TB/s) sustained by the inner loop as a function of the mean column distance
// between consecutive entries of a unit.  Round 1 took it from a microbenchmark (scripts/ubench_gap.hip: 4.4 TB/s at a gap
// of 1.5 falling to 2.4 at 12); with the hot-column table and the packed gather vector the real kernels lose far less to a
// wide gap, and the table made the planner split short-row graphs that run faster unsplit.  Round 3 re-fitted it to the
// kernels themselves (8 nnz / (launch - 10 us) on the stand-ins at 256 and 512 unsplit blocks, one box:
// hollywood 2.4 -> 5.8, orkut / ogbl-ppa 3.7 -> 5.75, products 5 -> 5.45 and 10 -> 4.9, pokec 13 -> 4.5 and 26 -> 3.8).
static double stream_rate(double gap) {
    static const double gx[] = {2.5, 5.0, 10.0, 13.0, 26.0, 52.0, 104.0};
    static const double gy[] = {5.85, 5.45, 4.9, 4.5, 3.8, 3.0, 2.3};
    if (gap <= gx[0]) return gy[0];
    for (int i = 1; i < 7; i++)
        if (gap <= gx[i]) {
            double t = (std::log(gap) - std::log(gx[i - 1])) / (std::log(gx[i]) - std::log(gx[i - 1]));
            return gy[i - 1] + t * (gy[i] - gy[i - 1]);
        }
    return gy[6];
}

// choose (#row blocks, #segments per block): blocks*segments ~ 256*k equal units, rows per block as
// large as LDS allows (dense column sweep => coalesced gathers) unless splitting costs more than it buys
static Shape choose_shape(uint64_t rows, uint64_t cols, uint64_t nnz, int num_cus) {
    Shape best{1, 1};
    if (rows == 0 || nnz == 0) return best;
    const double deg = (double)nnz / (double)rows;
    const uint64_t rmax = kMaxPlainRows - 64;   // slack: blocks are cut by nnz, not by row count
    double best_cost = 1e300;
    for (int k = 1; k <= 16 && best_cost > 1e299; k *= 2) {
        for (uint32_t S = 1; S <= 64; S++) {
            uint64_t B = (uint64_t)num_cus * k / S;
            if (B == 0) break;
            if (B > rows) B = rows;
            const uint64_t R = (rows + B - 1) / B;
            if (R > rmax) continue;
            const double gap = (double)cols / ((double)R * deg);
            const double flush = (S == 1) ? 0.0 : (double)rows * 4.0 * (2.0 * S + 1.0) / (8.0 * nnz);   // planes out + in, y
            const double util = (double)B * S / ((double)num_cus * k);
            // (a split plan pays its planes, the combine launch and a worse balance between units: measured ~8 us)
            const double t = (8.0 * nnz * (1.0 + flush)) / (stream_rate(gap) * 1e12) / util + 3.0e-6 * k + (S == 1 ? 0.0 : 8.0e-6);
            if (t < best_cost) {
                best_cost = t;
                best = Shape{(uint32_t)B, S};
            }
        }
    }
    if (best_cost > 1e299) best = Shape{(uint32_t)((rows + rmax - 1) / rmax), 1};  // taller than 16 rounds of CUs
    const long fb = debug_knob("spmv_blocks", 0), fs = debug_knob("spmv_segments", 0);
    if (fb > 0) best.blocks = (uint32_t)std::min<uint64_t>((uint64_t)fb, rows);
    if (fs > 0) best.segments = (uint32_t)std::min<long>(fs, 4096);
    return best;
}

// see gl_spmv_plan.h
BlockPlan plan_blocks(Shape shape, const uint32_t *h_indptr, uint32_t row_begin, uint32_t row_end, uint32_t max_rows,
                      uint32_t align) {
    BlockPlan bp;
    const uint64_t nz0 = h_indptr[row_begin], nz1 = h_indptr[row_end], nnz = nz1 - nz0;
    std::vector<uint32_t> &bstart = bp.bstart;
    bstart.push_back(row_begin);
    // Balance: the launch ends with its slowest unit, so the cuts minimise the LARGEST block (binary search on its size,
    // greedy fill) instead of tracking cumulative targets -- with whole-row cuts a block next to a hub row used to end up
    // several per cent over the mean (orkut stand-in: 765 K .. 888 K entries per block around a mean of 827 K, and the
    // 888 K unit finished 28 us after the average one in a 313 us launch).  GRAPHLILY_DEBUG spmv_balance=0: cumulative targets.
    if (nnz > 0 && debug_knob("spmv_balance", 1) != 0 && shape.blocks > 1) {
        // blocks needed when no block may hold more than `cap` entries (a single longer row gets a block of its own)
        auto cut = [&](uint64_t cap, std::vector<uint32_t> *out) -> uint32_t {
            uint32_t r = row_begin, made = 0;
            while (r < row_end) {
                const uint32_t hi = (uint32_t)std::min<uint64_t>(row_end, (uint64_t)r + max_rows);
                const uint64_t lim = (uint64_t)h_indptr[r] + cap;
                const uint32_t *ub = std::upper_bound(h_indptr + r + 1, h_indptr + hi + 1, (uint32_t)std::min<uint64_t>(lim, 0xffffffffull));
                uint32_t e = (uint32_t)(ub - h_indptr) - 1u;
                if (e < r + 1) e = r + 1;
                if (align > 1u && e < row_end) {
                    uint32_t ea = e / align * align;
                    if (ea <= r) ea = std::min<uint64_t>(row_end, (uint64_t)(r / align + 1u) * align);
                    e = ea;
                }
                if (out) out->push_back(e);
                r = e;
                made++;
            }
            return made;
        };
        uint64_t lo = (nnz + shape.blocks - 1) / shape.blocks, hi = nnz;   // smallest cap that needs <= shape.blocks blocks
        if (cut(hi, nullptr) > shape.blocks) {
            lo = hi;   // the row cap alone forces more blocks than planned: fill them as evenly as the cap allows
            const uint32_t forced = cut(hi, nullptr);
            uint64_t l2 = (nnz + forced - 1) / forced, h2 = nnz;
            while (l2 < h2) {
                const uint64_t mid = (l2 + h2) / 2;
                if (cut(mid, nullptr) <= forced) h2 = mid; else l2 = mid + 1;
            }
            lo = l2;
        } else {
            while (lo < hi) {
                const uint64_t mid = (lo + hi) / 2;
                if (cut(mid, nullptr) <= shape.blocks) hi = mid; else lo = mid + 1;
            }
        }
        cut(lo, &bstart);
    } else if (nnz > 0) {
        const double target = (double)nnz / (double)shape.blocks;
        uint32_t r = row_begin, made = 0;
        while (r < row_end) {
            made++;
            const uint32_t hi = (uint32_t)std::min<uint64_t>(row_end, (uint64_t)r + max_rows);
            uint32_t e;
            if (made >= shape.blocks && hi == row_end) {
                e = row_end;   // the last planned block takes what is left if it fits
            } else {
                const uint64_t want64 = nz0 + (uint64_t)std::llround(target * made);
                const uint32_t want = (uint32_t)std::min<uint64_t>(want64, nz1);
                // last e in [r+1, hi] with indptr[e] <= want, at least one row
                const uint32_t *ub = std::upper_bound(h_indptr + r + 1, h_indptr + hi + 1, want);
                e = (uint32_t)(ub - h_indptr) - 1u;
                if (e < r + 1) e = r + 1;
                if (align > 1u) {   // interior boundaries on multiples of `align` rows (row_begin and max_rows are)
                    uint32_t ea = (e + align / 2u) / align * align;
                    if (ea <= r) ea = r - r % align + align;
                    if (ea >= hi) ea = (hi == row_end) ? row_end : hi / align * align;
                    e = ea;
                }
            }
            bstart.push_back(e);
            r = e;
        }
    }
    const uint32_t nblocks = bp.nblocks = (uint32_t)bstart.size() - 1;
    // The planner asked for shape.blocks x shape.segments units; the row cap can have produced more blocks
    // than planned, so the unit budget (a multiple of the CU count) is re-distributed over the actual
    // blocks in proportion to their non-zeros.
    bp.seg.assign(nblocks, 1);
    if (nblocks && shape.segments > 1) {
        const uint32_t cus = (uint32_t)ctx().num_cus;
        uint64_t budget = (uint64_t)shape.blocks * shape.segments;
        budget = std::max<uint64_t>(cus, budget / cus * cus);           // whole rounds of workgroups
        if (budget < nblocks) budget = nblocks;
        const double per_unit = (double)nnz / (double)budget;
        uint64_t used = 0;
        std::vector<std::pair<double, uint32_t>> frac;
        for (uint32_t b = 0; b < nblocks; b++) {
            const double want = (double)((uint64_t)h_indptr[bstart[b + 1]] - h_indptr[bstart[b]]) / per_unit;
            bp.seg[b] = std::max<uint32_t>(1u, (uint32_t)want);
            used += bp.seg[b];
            frac.push_back({want - (double)bp.seg[b], b});
        }
        std::sort(frac.begin(), frac.end(), [](const std::pair<double, uint32_t> &x, const std::pair<double, uint32_t> &y) { return x.first > y.first; });
        for (size_t i = 0; used < budget && i < frac.size(); i++, used++) bp.seg[frac[i].second]++;
        for (uint32_t b = 0; b < nblocks; b++) bp.Smax = std::max(bp.Smax, bp.seg[b]);
    }
    bp.all_direct = (bp.Smax == 1);
    bp.unit_of.assign(bp.Smax, std::vector<uint32_t>(nblocks, 0xffffffffu));
    for (uint32_t sgm = 0; sgm < bp.Smax; sgm++)
        for (uint32_t b = 0; b < nblocks; b++)
            if (bp.seg[b] > sgm) bp.unit_of[sgm][b] = bp.nunits++;
    return bp;
}

// ------------------------------------------------------------------------------------- plan creation
struct PlanDeleter {
    void operator()(gl_spmv_plan p) const { gl_spmv_plan_destroy(p); }
};
using PlanOwner = std::unique_ptr<gl_spmv_plan_s, PlanDeleter>;   // a plan under construction: freed on every error exit

// the planner's GRAPHLILY_DEBUG overrides (gl_common.h), read once per plan
struct Knobs {
    long pattern = debug_knob("spmv_pattern", 1);      // 0: no pattern layout
    long hot = debug_knob("spmv_hot", 1);              // 0: no hot table, > 1: its size
    long hot_floor = debug_knob("spmv_hot_floor", LONG_MIN);   // a hot column's degree per row block (unset: 1 pattern, 4 general)
    long helper = debug_knob("spmv_helper", -1);       // -1 automatic, 0 gather, 1 spread, 2 self-hot (if possible)
    long compact = debug_knob("spmv_compact", 1);      // 0: no packed vector, 2: one degree class, 3: packed even where self-hot
    long hub_div = debug_knob("spmv_hub_div", 48);
    long mix = debug_knob("spmv_mix", -1);
    long boolean = debug_knob("spmv_bool", 1);
};

// the caller's CSR, of which the plan covers rows [row_begin, row_end)
struct HostCsr {
    const uint32_t *indptr, *indices;
    const float *data;
    uint32_t num_cols, row_begin, row_end;
    uint64_t nnz;
};

static int column_error(uint32_t num_cols) {
    return set_error(GL_ERR_INVALID_ARG, "gl_spmv_plan_create: column index out of range (num_cols %u)", num_cols);
}

// GL_PLAN_REFERENCE_ORDER: the shard's CSR as it is (diagnostic layout, spmv_reference_order_kernel)
static int plan_reference_order(gl_spmv_plan p, const HostCsr &a) {
    const uint64_t nz0 = a.indptr[a.row_begin], nnz = a.nnz;
    for (uint64_t i = nz0; i < nz0 + nnz; i++)
        if (a.indices[i] >= a.num_cols) return column_error(a.num_cols);
    p->reference_order = true;
    const uint32_t rows = a.row_end - a.row_begin;
    std::vector<uint32_t> ip((size_t)rows + 1u);
    for (uint32_t r = 0; r <= rows; r++) ip[r] = (uint32_t)(a.indptr[a.row_begin + r] - nz0);
    hipError_t e = hipMalloc((void **)&p->d_csr_indptr, ip.size() * 4u);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_csr_indices, std::max<uint64_t>(nnz, 1u) * 4u);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_csr_data, std::max<uint64_t>(nnz, 1u) * 4u);
    if (e == hipSuccess) e = hipMemcpy(p->d_csr_indptr, ip.data(), ip.size() * 4u, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(p->d_csr_indices, a.indices + nz0, nnz * 4u, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(p->d_csr_data, a.data + nz0, nnz * 4u, hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_error(GL_ERR_HIP, "gl_spmv_plan_create: reference-order plan: %s", hipGetErrorString(e));
    p->device_bytes = ip.size() * 4u + nnz * 8u;
    return GL_OK;
}

// host twin of fmt_detect_pattern (gl_format.hip)
static int detect_pattern_host(const HostCsr &a, std::vector<uint32_t> &colbits, std::vector<uint32_t> &diag_has,
                               std::vector<float> &diag_val, int *mismatch_out, uint64_t *exceptions_out) {
    const uint32_t num_cols = a.num_cols, row_begin = a.row_begin, row_end = a.row_end, rows = row_end - row_begin;
    const uint32_t *h_indptr = a.indptr, *h_indices = a.indices;
    const float *h_data = a.data;
    int mismatch = 0;
    uint64_t exceptions = 0;
    colbits.assign(num_cols, 0u);
    diag_has.assign((size_t)(rows + 31) / 32, 0u);
    diag_val.assign(rows, 0.0f);
    // pass 1: any writer wins (all of a column's writers agree if the column is constant); pass 2 verifies
#pragma omp parallel for schedule(static, 4096)
    for (int64_t r = row_begin; r < (int64_t)row_end; r++)
        for (uint64_t i = h_indptr[r]; i < h_indptr[r + 1]; i++) {
            const uint32_t c = h_indices[i];
            // write only when it changes something: hub columns are written from every thread's row range, and
            // unconditional stores would bounce their cache lines between all cores
            if (c < num_cols && c != (uint32_t)r) {
                const uint32_t bits = __builtin_bit_cast(uint32_t, h_data[i]);
                if (__atomic_load_n(&colbits[c], __ATOMIC_RELAXED) != bits) __atomic_store_n(&colbits[c], bits, __ATOMIC_RELAXED);
            }
        }
#pragma omp parallel for schedule(static, 4096) reduction(| : mismatch) reduction(+ : exceptions)
    for (int64_t r = row_begin; r < (int64_t)row_end; r++) {   // 4096 rows = whole diag_has words per thread
        uint32_t nexc = 0;
        for (uint64_t i = h_indptr[r]; i < h_indptr[r + 1]; i++) {
            const uint32_t c = h_indices[i], bits = __builtin_bit_cast(uint32_t, h_data[i]);
            if (c >= num_cols) { mismatch = 1; continue; }
            if (colbits[c] == bits) continue;             // a regular entry of its column (diagonal or not)
            if (c != (uint32_t)r) { mismatch = 1; continue; }
            nexc++;                                        // diagonal entry that differs from its column's value
            diag_val[r - row_begin] = h_data[i];
            diag_has[(r - row_begin) >> 5] |= 1u << ((r - row_begin) & 31);
        }
        if (nexc > 1) mismatch = 1;   // several different diagonal values in one row: keep the general layout
        exceptions += nexc;
    }
    *mismatch_out = mismatch;
    *exceptions_out = exceptions;
    return GL_OK;
}

// host twin of fmt_values_finite (gl_format.hip): no stored value of the shard is +-inf / NaN
static bool values_finite_host(const HostCsr &a) {
    const uint64_t nz0 = a.nnz ? a.indptr[a.row_begin] : 0;
    int found = 0;
#pragma omp parallel for schedule(static) reduction(| : found)
    for (int64_t i = 0; i < (int64_t)a.nnz; i++)
        found |= (__builtin_bit_cast(uint32_t, a.data[nz0 + i]) & 0x7f800000u) == 0x7f800000u;
    return !found;
}

// host twin of fmt_column_degrees (gl_format.hip): non-zeros per column within the shard
static int column_degrees_host(const HostCsr &a, std::vector<uint32_t> &deg, int *bad_col) {
    const uint64_t nz0 = a.indptr[a.row_begin];
    deg.assign(a.num_cols, 0);
    // sequential on purpose: atomics from all cores pile up on the hub columns' counters (measured slower)
    for (uint64_t i = nz0; i < nz0 + a.nnz; i++) {
        if (a.indices[i] < a.num_cols) deg[a.indices[i]]++;
        else *bad_col = 1;
    }
    return GL_OK;
}

// The H highest-degree columns of the shard get an LDS-resident copy of x: H = what fits next to the tallest f64 tile (incl.
// worst-case hub slots).  hot_cols: slot -> column; colmap[c] = 0x80000000 | slot for every hot column c
static void choose_hot_columns(const Knobs &k, uint32_t flags, uint64_t nnz, const std::vector<uint32_t> &deg, uint32_t tallest,
                               uint32_t nblocks, bool pattern, std::vector<uint32_t> &hot_cols, std::vector<uint32_t> &colmap) {
    const uint32_t num_cols = (uint32_t)deg.size();
    // 8-byte accumulators unless the caller promised to run only the 4-byte-tile semirings
    const size_t elem = (flags & (GL_PLAN_NO_MULADD | GL_PLAN_BOOLEAN)) ? sizeof(float) : sizeof(double);
    const size_t tile_bytes = ((size_t)tallest + kHubSlots * kMaxHubRows + kPadSlots) * elem;   // (+ the dummy slots of padding entries)
    // as many columns as fit next to the tallest tile (whole wavefronts of slots), at most 32 K
    uint32_t room = 0;
    if (tile_bytes + 4096u <= kLdsBudget)
        room = std::min<uint32_t>(1u << 15, (uint32_t)((kLdsBudget - tile_bytes - 320u) / 4u / 64u * 64u));   // (- the 64 identity slots, the ticket word, rounding)
    uint32_t H = room;
    // Round 4, same-box sweeps of the table size (profiles/r04_small_graph_ab.txt): with the packed gather vector ordered by
    // degree class the popular columns are cheap to gather anyway, and the table has a price per workgroup (its copy in the
    // prologue, an LDS look-up per entry).  From 100 M non-zeros on the size hardly matters (+-1 %); below 64 M the first
    // 1-2 K columns are all that pays (ogbl-ppa stand-in 61.8 -> 64.4 % of peak, pokec 49.8 -> 49.8); and a short stream
    // whose whole x fits a corner of the L2 (googleplus stand-in: 432 KB) runs fastest with no table (57.5 -> 65.2 %).
    // Round 5: run-coded hot entries cost 6.19 (2.19) bytes and no gather, delta-coded cold ones 7 (3) + a gather -- the cap of
    // 2048 columns below 64 M non-zeros no longer pays (profiles/r05_hot_table_sweep.txt: ogbl-ppa general 0.068 -> 0.062 ms,
    // pattern 0.049 -> 0.044 with the 6464 columns the degree floor admits; pokec and the community stand-in flat); the short
    // stream with a tiny x still runs fastest without a table (googleplus 0.016 against 0.017-0.018 ms).
    if (nnz <= (16ull << 20) && (uint64_t)num_cols * 4u <= (1ull << 20)) H = 0;
    if (k.hot > 1) H = std::min<uint32_t>(room, (uint32_t)k.hot);
    if (!H) return;
    const uint32_t dmax = num_cols ? *std::max_element(deg.begin(), deg.end()) : 0u;
    std::vector<uint32_t> hist((size_t)dmax + 2, 0);
    for (uint32_t c = 0; c < num_cols; c++) hist[deg[c]]++;
    // thr = smallest degree such that at most H columns have degree >= thr; a column must also
    // appear often enough to be worth a slot (>= 4 entries per row block on average)
    // (round 6: a ROW-PACKED hot entry -- pattern plans -- costs 2.3 bytes, a seventh of an LDS atomic and no gather: every
    //  column that averages one entry per row block is worth a slot there; profiles/r06_hot_floor_sweep.txt: ogbl-ppa
    //  0.037 -> 0.034 ms, pokec 0.041 -> 0.040, the table-size-limited stand-ins unchanged)
    const long floor_knob = k.hot_floor != LONG_MIN ? k.hot_floor : (pattern ? 1 : 4);
    const uint32_t floor_deg = std::max<uint32_t>(8u, (uint32_t)floor_knob * nblocks);
    uint64_t seen = 0;
    uint32_t thr = dmax + 1;
    while (thr > floor_deg && seen + hist[thr - 1] <= H) { thr--; seen += hist[thr]; }
    std::vector<uint32_t> hot;
    for (uint32_t c = 0; c < num_cols; c++)
        if (deg[c] >= thr && hot.size() < H) hot.push_back(c);
    uint64_t hn = 0;
    for (uint32_t c : hot) hn += deg[c];
    if (hot.empty() || (double)hn < 0.05 * (double)nnz) return;   // not worth the table
    for (uint32_t j = 0; j < (uint32_t)hot.size(); j++) colmap[hot[j]] = 0x80000000u | j;
    hot_cols.swap(hot);
}

// The packed gather vector.  Gathers cost per distinct 128-byte line a wavefront instruction touches (~2 clocks), and a row
// block's sweep touches every line of x that holds one of its cold columns -- with arbitrary vertex labels, all of them.  So the
// cold entries index a packed copy of x instead (general plans: xc[j] = x[ccols[j]], filled by the per-run helper kernel;
// pattern plans: z is simply built in that order) which
//   - drops the columns that are never gathered: no entry in this shard (isolated vertices; most low-degree columns of a 1/8
//     row shard) or served from the hot table;
//   - orders the rest by degree class (>= nblocks/4, /16, /64, below; ascending column inside a class, so the helper's reads
//     stay nearly sequential): a line of 32 rare columns is then touched by few row blocks instead of riding along with a
//     popular neighbour in every one.
// Lines touched per block sweep on the ogbn-products stand-in: 68.7 K (x) -> 48.5 K (packed) -> 29.2 K (classes); a full sort
// by degree gives 28.5 K.  ccols: packed index -> column; colmap[c] of a cold column c becomes its packed index (0xffffffff: never
// gathered)
static void order_packed_columns(const std::vector<uint32_t> &deg, const BlockPlan &bp, bool by_class, std::vector<uint32_t> &ccols,
                                 std::vector<uint32_t> &colmap) {
    const uint32_t num_cols = (uint32_t)deg.size(), nb = bp.nblocks;
    const uint32_t edge[3] = {std::max(nb / 4u, 1u), std::max(nb / 16u, 1u), std::max(nb / 64u, 1u)};
    auto cls = [&](uint32_t c) -> int {
        if (deg[c] == 0 || (colmap[c] >> 31)) return -1;   // never gathered
        // split blocks keep one class: their segments cut the stream by position, and a segment of rare columns
        // only would touch several times the lines of its siblings (1/8 orkut shard: 0.061 -> 0.082 ms with classes)
        if (!by_class) return 0;
        return deg[c] >= edge[0] ? 0 : deg[c] >= edge[1] ? 1 : deg[c] >= edge[2] ? 2 : 3;
    };
    uint32_t start[5] = {0, 0, 0, 0, 0};
    for (uint32_t c = 0; c < num_cols; c++) {
        const int k = cls(c);
        if (k >= 0) start[k + 1]++;
    }
    for (int k = 0; k < 4; k++) start[k + 1] += start[k];
    const uint32_t gathered = start[4];
    ccols.assign(std::max(gathered, 1u), 0u);   // (every entry hot: keep the arrays non-empty)
    for (uint32_t c = 0; c < num_cols; c++) {
        const int k = cls(c);
        if (k >= 0) {
            colmap[c] = start[k];
            ccols[start[k]++] = c;
        } else if (!(colmap[c] >> 31)) {
            colmap[c] = 0xffffffffu;
        }
    }
}

// host twin of fmt_emit_general (gl_format.hip): the per-block column sort, group packing and emission with OpenMP
static int emit_general_host(const HostCsr &a, const EmitGeneral &eg, gl_spmv_plan p, std::vector<uint32_t> &hub_count, uint64_t *hot_nnz_out) {
    const uint32_t *h_indptr = a.indptr, *h_indices = a.indices, *colmap = eg.colmap, *colbits = eg.colbits;
    const float *h_data = a.data;
    const BlockPlan &bp = *eg.bp;
    const std::vector<uint32_t> &bstart = bp.bstart, &seg = bp.seg;
    const std::vector<std::vector<uint32_t>> &unit_of = bp.unit_of;
    const uint32_t nblocks = bp.nblocks, nunits = bp.nunits, gather_cols = eg.gather_cols, nhot_table = eg.nhot_table;
    const bool all_direct = bp.all_direct, pattern = eg.pattern, diag_mode = eg.diag_mode;
    // the delta-coded cold stream and the run-coded hot stream, both in elements of 4 (pattern: 8) lane-interleaved groups
    const uint32_t cold_groups = pattern ? kColdGroupsPattern : kColdGroupsGeneral;   // units hold whole elements
    const uint32_t cold_elem_bytes = pattern ? kColdElemBytesPattern : kColdElemBytesGeneral;
    // pattern plans carry the ROW-PACKED hot stream (gl_spmv_plan.h): an element = 64 records of 7 table slots + a row slot, no
    // headers, no present lists; general plans the run-coded one
    const bool hot_rows = pattern;
    const uint32_t hot_groups = hot_rows ? 1u : kHotGroupsGeneral;
    const uint32_t hot_elem_bytes = hot_rows ? kHotElemBytesRows : kHotElemBytesGeneral;
    const uint32_t hot_hdr_words = hot_rows ? 0u : kHotHdrWordsPerGroup * hot_groups;

    // ---- pass 1: cold / hot entries per block, from which every unit's place in the arrays follows (layout_units)
    std::vector<uint64_t> mc(nblocks, 0), mh(nblocks, 0), mrec(nblocks, 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t b = 0; b < (int64_t)nblocks; b++) {
        uint64_t nc = 0, nh = 0, nrec = 0;
        for (uint32_t r = bstart[b]; r < bstart[b + 1]; r++) {
            uint64_t hr = 0;
            for (uint64_t i = h_indptr[r]; i < h_indptr[r + 1]; i++) {
                const uint32_t c = h_indices[i];   // (out-of-range columns were reported by the degree pass)
                if (diag_mode && c == r && __builtin_bit_cast(uint32_t, h_data[i]) != colbits[c]) continue;
                if (colmap[c] >> 31) hr++; else nc++;
            }
            nh += hr;
            nrec += (hr + kHotRecEntries - 1u) / kHotRecEntries;   // row-packed hot stream: records of <= 7 entries of one row
        }
        mc[b] = nc, mh[b] = nh, mrec[b] = nrec;
    }
    const UnitLayout ul = layout_units(bp, mc, mh, eg.dummy_max, hot_groups, nhot_table, hot_rows ? &mrec : nullptr);
    const uint64_t total_groups = ul.cold_goff[nunits], hot_elems = ul.hot_e0[nunits];
    if (!(total_groups < 0xffffffffull && hot_elems < 0xffffffffull && ul.present_off[nunits] < 0xffffffffull))
        return set_error(GL_ERR_INVALID_ARG, "gl_spmv_plan_create_ex: invalid argument: total_groups < 0xffffffffull && "
                         "hot_elems < 0xffffffffull && ul.present_off[nunits] < 0xffffffffull");
    // cold elements with one element of slack behind them (clamped loads); slots of the slack are never accumulated
    std::vector<unsigned char> entries((size_t)(total_groups / cold_groups + 1) * cold_elem_bytes, 0);
    std::vector<uint32_t> bases(total_groups, 0u);
    std::vector<uint4> units((size_t)nunits * 3);
    std::vector<uint32_t> hub_rows((size_t)nblocks * kMaxHubRows, 0);   // slot b*kMaxHubRows + h
    // hot arrays with one element of slack behind them (the kernel's clamped loads land there; never accumulated)
    std::vector<unsigned char> hot_bytes((size_t)(hot_elems + 1) * hot_elem_bytes, 0);
    {
        uint16_t *rows16 = reinterpret_cast<uint16_t *>(hot_bytes.data() + (size_t)hot_elems * hot_elem_bytes);
        for (uint32_t k = 0; k < (hot_rows ? hot_elem_bytes / 2u : 64u * hot_groups); k++) rows16[k] = (uint16_t)kRowPad;
    }
    std::vector<uint32_t> hot_hdr(hot_rows ? (size_t)8 : (size_t)(hot_elems + 1) * hot_hdr_words, 0u);
    std::vector<uint16_t> present((size_t)std::max<uint64_t>(ul.present_off[nunits], 2u), 0);
    uint32_t max_present = 0;
    uint64_t hot_nnz = 0;
#pragma omp parallel reduction(+ : hot_nnz) reduction(max : max_present)
    {
        std::vector<Rec> recs, tmp, hot;
        std::vector<uint64_t> rec_of_hot;      // row-packed hot stream: the block's record each hot entry belongs to
#pragma omp for schedule(dynamic, 1)
        for (int64_t b = 0; b < (int64_t)nblocks; b++) {
            const uint32_t r0 = bstart[b], r1 = bstart[b + 1];
            recs.clear();
            hot.clear();
            for (uint32_t r = r0; r < r1; r++)
                for (uint64_t i = h_indptr[r]; i < h_indptr[r + 1]; i++) {
                    const uint32_t c = h_indices[i];
                    const uint32_t v = __builtin_bit_cast(uint32_t, h_data[i]);
                    if (diag_mode && c == r && v != colbits[c]) continue;   // the row's diagonal exception lives in diag_val
                    if (colmap[c] >> 31) hot.push_back(Rec{colmap[c] & 0x7fffffffu, r - r0, v});
                    else recs.push_back(Rec{colmap[c], r - r0, v});
                }
            sort_by_col(recs, tmp, gather_cols);
            if (!hot_rows) sort_by_col(hot, tmp, nhot_table ? nhot_table : 1u);   // by slot: a column's entries form a run
            // (row-packed stream: `hot` stays as it was collected -- rows ascending, a row's entries in CSR order)
            hot_nnz += hot.size();
            const uint64_t mcb = recs.size(), m = mcb + hot.size();
            // hub rows: a large share of the block's entries (=> several lanes of every step on one LDS word)
            std::vector<uint32_t> cnt(r1 - r0, 0);
            for (const Rec &rc : recs) cnt[rc.row_local]++;
            for (const Rec &rc : hot) cnt[rc.row_local]++;
            std::vector<int> hub_of(r1 - r0, -1);
            {
                const uint64_t thr = std::max<uint64_t>(256, m / (uint64_t)eg.hub_div);
                uint32_t nh = 0;
                for (uint32_t i = 0; i < r1 - r0 && nh < kMaxHubRows; i++)
                    if (cnt[i] >= thr) {
                        hub_of[i] = (int)nh;
                        hub_rows[(size_t)b * kMaxHubRows + nh] = i;
                        nh++;
                    }
                hub_count[b] = nh;
            }
            const uint32_t nrows_b = r1 - r0;
            // padding entries accumulate into the slots behind the block's last one (dummies nobody reads, one per lane): the
            // kernel's accumulates need no test
            const uint32_t pad_slot = nrows_b + kHubSlots * hub_count[b];
            // the block's cold entries (column-sorted) and hot entries (slot-sorted) are each cut into S pieces
            auto slot_of = [&](const Rec &rc, uint32_t fill) -> uint32_t {
                const int hb = hub_of[rc.row_local];
                return hb < 0 ? rc.row_local : nrows_b + kHubSlots * (uint32_t)hb + (fill & (kHubSlots - 1u));
            };
            const uint32_t S = seg[b];
            for (uint32_t s = 0; s < S; s++) {
                const size_t u = unit_of[s][b];
                const uint64_t goff = ul.cold_goff[u];
                // ---- the unit's cold entries, delta-coded (gl_spmv_plan.h): position q of the unit's stream = lane q % 64 of
                //      group goff + q / 64
                uint64_t q = 0;
                uint32_t prev = 0;
                auto put = [&](uint32_t idx, uint32_t slot, uint32_t val) {
                    const uint64_t g = goff + q / 64;
                    const uint32_t lane = (uint32_t)(q % 64), k = (uint32_t)(g % cold_groups);
                    unsigned char *el = entries.data() + (size_t)(g / cold_groups) * cold_elem_bytes;
                    const uint32_t delta = lane ? idx - prev : 0u;     // (a group's first entry: its index is the group's base)
                    if (!lane) bases[g] = idx;
                    if (pattern) {
                        reinterpret_cast<uint16_t *>(el)[lane * 8u + k] = (uint16_t)slot;
                        el[1024u + lane * 8u + k] = (unsigned char)delta;
                    } else {
                        reinterpret_cast<uint16_t *>(el)[lane * 4u + k] = (uint16_t)slot;
                        el[512u + lane * 4u + k] = (unsigned char)delta;
                        reinterpret_cast<uint32_t *>(el + 768u)[lane * 4u + k] = val;
                    }
                    prev = idx;
                    q++;
                };
                for (uint64_t i = mcb * s / S; i < mcb * (s + 1) / S; i++) {
                    const Rec &rc = recs[i];
                    if (q)   // dummy entries (a dummy slot, value 0) bridge a gap of more than 255 columns, 255 at a time
                        while (rc.col - prev > kColdMaxDelta) put(prev + kColdMaxDelta, pad_slot + (uint32_t)(q % 64), 0u);
                    put(rc.col, slot_of(rc, (uint32_t)(q % 64)), rc.val);
                }
                // padding up to whole elements: dummy slots, delta 0 (all-padding groups: base 0)
                const uint64_t qend = (q + 64u * cold_groups - 1) / (64u * cold_groups) * (64u * cold_groups);
                while (q < qend) {
                    if (q % 64 == 0) prev = 0;
                    put(prev, pad_slot + (uint32_t)(q % 64), 0u);
                }
                const uint64_t g = goff + q / 64;
                const uint32_t ncold = (uint32_t)(g - goff);
                if (hot_rows) {
                    // ---- the unit's hot entries, ROW-PACKED (gl_spmv_plan.h): the block's records -- <= 7 entries of one row
                    //      each, rows ascending -- are cut into the block's units by position; a unit's records are dealt to the
                    //      lanes in 64 contiguous chunks: element e, lane l = record l * chunk + e
                    const uint64_t M = mrec[b], j0 = M * s / S, j1 = M * (s + 1) / S, e0 = ul.hot_e0[u];
                    const uint32_t nel = (uint32_t)(ul.hot_e0[u + 1] - e0), chunk = nel;
                    for (uint32_t e = 0; e < nel; e++) {      // every field starts as padding: the identity slot, the lane's dummy row
                        uint16_t *el = reinterpret_cast<uint16_t *>(hot_bytes.data() + (size_t)(e0 + e) * hot_elem_bytes);
                        for (uint32_t l = 0; l < 64u; l++) {
                            for (uint32_t k = 0; k < kHotRecEntries; k++) el[l * 8u + k] = (uint16_t)nhot_table;
                            el[l * 8u + 7u] = (uint16_t)(pad_slot + l);
                        }
                    }
                    // record j of the block = the (j - rec_first[row])-th group of 7 of its row's hot entries: walk the block's
                    // hot list once, keeping the record counter
                    if (s == 0) {
                        rec_of_hot.clear();
                        uint64_t j = 0;
                        for (size_t i = 0; i < hot.size();) {
                            size_t i1 = i;
                            while (i1 < hot.size() && hot[i1].row_local == hot[i].row_local) i1++;
                            for (size_t q = i; q < i1; q++) rec_of_hot.push_back(j + (q - i) / kHotRecEntries);
                            j += (i1 - i + kHotRecEntries - 1u) / kHotRecEntries;
                            i = i1;
                        }
                    }
                    for (size_t i = 0, f = 0; i < hot.size(); i++) {
                        const uint64_t j = rec_of_hot[i];
                        f = (i > 0 && rec_of_hot[i - 1] == j) ? f + 1 : 0;   // field = position inside the record
                        if (j < j0 || j >= j1) continue;
                        const uint32_t jj = (uint32_t)(j - j0), l = jj / chunk, e = jj % chunk;
                        uint16_t *rec = reinterpret_cast<uint16_t *>(hot_bytes.data() + (size_t)(e0 + e) * hot_elem_bytes) + l * 8u;
                        rec[f] = (uint16_t)hot[i].col;                       // the plan's (global) hot slot
                        if (f == 0) rec[7] = (uint16_t)slot_of(hot[i], l);   // hub rows: private slot by lane
                    }
                    units[3 * u] = make_uint4((uint32_t)goff, ncold, r0, (r1 - r0) | (all_direct ? 0x80000000u : 0u));
                    units[3 * u + 1] = make_uint4((uint32_t)((size_t)b * kMaxHubRows), hub_count[b], nel, s);
                    units[3 * u + 2] = make_uint4((uint32_t)e0, 0u, nhot_table, 0u);
                    continue;
                }
                // ---- the unit's hot entries, run-coded (gl_spmv_plan.h)
                const uint64_t h0 = hot.size() * s / S, h1 = hot.size() * (s + 1) / S, e0 = ul.hot_e0[u];
                uint16_t *pres = present.data() + ul.present_off[u];
                uint32_t np = 0;
                for (size_t e = (size_t)e0; e < (size_t)ul.hot_e0[u + 1]; e++) {   // every slot of the unit's elements starts as padding
                    uint16_t *rows16 = reinterpret_cast<uint16_t *>(hot_bytes.data() + e * hot_elem_bytes);
                    for (uint32_t k = 0; k < 64u * hot_groups; k++) rows16[k] = (uint16_t)(pad_slot + k / hot_groups);   // (lane k / HG)
                }
                for (uint64_t i = h0; i < h1; i++) {
                    const uint64_t j = i - h0, hg = j / 64;
                    const uint32_t l = (uint32_t)(j % 64), k = (uint32_t)(hg % hot_groups);
                    const size_t e = (size_t)(e0 + hg / hot_groups);
                    const bool start = i == h0 || hot[i].col != hot[i - 1].col;
                    if (start) pres[np++] = (uint16_t)hot[i].col;
                    uint32_t *hd = hot_hdr.data() + e * hot_hdr_words;
                    if (l == 0) hd[2 * hot_groups + k] = np - 1u;                               // the group's first table slot
                    else if (start) hd[2 * k + ((l - 1u) >> 5)] |= 1u << ((l - 1u) & 31u);      // bit l - 1: entry l starts a run
                    unsigned char *el = hot_bytes.data() + e * hot_elem_bytes;
                    const uint16_t slot16 = (uint16_t)slot_of(hot[i], l);
                    if (pattern) {
                        reinterpret_cast<uint16_t *>(el)[l * 8u + k] = slot16;
                    } else {
                        reinterpret_cast<uint16_t *>(el)[l * 4u + k] = slot16;
                        reinterpret_cast<uint32_t *>(el + 512)[l * 4u + k] = hot[i].val;
                    }
                }
                max_present = std::max(max_present, np);
                const uint32_t nhotg = (uint32_t)(ul.hot_e0[u + 1] - e0) * hot_groups;
                units[3 * u] = make_uint4((uint32_t)goff, ncold, r0, (r1 - r0) | (all_direct ? 0x80000000u : 0u));
                units[3 * u + 1] = make_uint4((uint32_t)((size_t)b * kMaxHubRows), hub_count[b], nhotg, s);
                units[3 * u + 2] = make_uint4((uint32_t)e0, (uint32_t)ul.present_off[u], np, 0u);
            }
        }
    }
    p->nhot_elems = hot_elems;
    p->nhot_lds = hot_rows ? (nhot_table ? nhot_table + 64u : 0u) : (max_present + 63u) / 64u * 64u;   // (rows: the whole table + the identity slots)
    p->ngroups = total_groups;
    *hot_nnz_out = hot_nnz;
    // one element of slack: the kernel's loads are unconditional and clamp to a unit's last element, which for a unit
    // without groups is the element that follows it
    bases.insert(bases.end(), 8, 0u);
    int rc;
    if ((rc = plan_upload(p, p->d_entries, entries.data(), entries.size())) != GL_OK ||
        (rc = plan_upload(p, p->d_bases, bases.data(), bases.size() * sizeof(uint32_t))) != GL_OK ||
        (rc = plan_upload(p, p->d_units, units.data(), units.size() * sizeof(uint4))) != GL_OK ||
        (rc = plan_upload(p, p->d_hub_rows, hub_rows.data(), hub_rows.size() * sizeof(uint32_t))) != GL_OK ||
        (rc = plan_upload(p, p->d_hot, hot_bytes.data(), hot_bytes.size())) != GL_OK ||
        (rc = plan_upload(p, p->d_hot_hdr, hot_hdr.data(), hot_hdr.size() * sizeof(uint32_t))) != GL_OK ||
        (rc = plan_upload(p, p->d_present, present.data(), present.size() * sizeof(uint16_t))) != GL_OK)
        return rc;
    p->b_entries = entries.size();
    p->b_bases = bases.size() * sizeof(uint32_t);
    p->b_units = units.size() * sizeof(uint4);
    p->b_hub_rows = hub_rows.size() * sizeof(uint32_t);
    p->b_hot = hot_bytes.size();
    p->b_hot_hdr = hot_hdr.size() * sizeof(uint32_t);
    p->b_present = present.size() * sizeof(uint16_t);
    return GL_OK;
}

// cold + hot stream elements per wavefront iteration (cold and hot elements hold the same number of groups): 2 + 1 (mix 2) or 1 + 1
// (mix 3).  Rounds past the end of the shorter stream touch only the other one.  Swept on every stand-in
// (profiles/r05_mix_sweep_delta_cold.txt, r05_mix_sweep_small_graphs.txt; 3 + 1 and 1 + 2 lost everywhere but one tie and are
// gone): general layout -- orkut (34 % hot) 0.275 ms at 2 + 1, 0.297 at 1 + 1; hollywood (61 %) 0.137 / 0.134; products (36 %)
// 0.179 / 0.178 -- pattern layout 1 + 1 everywhere (products 0.138 -> 0.130, pokec 0.048 -> 0.045).
static int choose_mix(const Knobs &k, bool pattern, bool have_hot, uint64_t hot_nnz, uint64_t nnz) {
    const double hot_frac = nnz ? (double)hot_nnz / (double)nnz : 0.0;
    // (profiles/r05_mix_sweep_small_graphs.txt: three cold elements per step are too many -- ogbl-ppa general 0.068 ms at 3 + 1,
    //  0.062 at 2 + 1, 0.064 at 1 + 1; the pattern layout, whose elements hold 8 groups, is fastest at 1 + 1 even where a
    //  quarter of the entries are hot: pokec 0.051 / 0.048 / 0.045, ogbl-ppa 0.049 / 0.046 / 0.043)
    const int mix = (pattern || hot_frac >= 0.42) ? 3 : 2;
    return !have_hot ? 0 : (k.mix > 0 ? (int)k.mix : mix);   // 0 would skip the hot groups
}

// The self-hot rule: a short stream (the whole sweep takes a few tens of microseconds) whose hot table is small enough for
// every workgroup to gather it from x in its prologue needs no helper launch -- nor, unless spmv_compact=3 asks for it, the
// packed vector that the helper would fill (googleplus stand-in: 23.7 -> 22.8 us)
static bool self_hot_rule(long helper_mode, uint64_t nnz, uint32_t nhot_table) {
    return (helper_mode == 2 || (helper_mode < 0 && nnz <= (16ull << 20))) && nhot_table <= 4096u;
}

// How the hot table / packed vector are refilled per run (launch_spmv):
//   self-hot   the self-hot rule holds and the plan has no packed vector: every workgroup gathers the table from x itself;
//   spread     a quarter or more of the columns are gathered: one streaming pass over x (spmv_spread_x_kernel);
//   gather     otherwise (sparse shards): spmv_hot_gather_kernel / spmv_prescale_kernel read only what they need.
struct Helper {
    bool self_hot, spread;
};
static Helper choose_helper(long mode, bool self_hot_ok, bool pattern, bool compact, uint32_t Smax, uint32_t gather_cols,
                            uint32_t nhot_table, uint32_t num_cols) {
    Helper h;
    h.self_hot = self_hot_ok && !pattern && !compact;   // (pattern plans always need their helper: it forms z = colval (x) x)
    // (split plans keep one ascending class, which the gathering kernels already read sequentially: pokec stand-in
    //  0.0742 ms gathered, 0.0760 ms spread; unsplit plans: equal on the general layout, orkut pattern layout 0.2146 -> 0.2102)
    h.spread = compact && (mode == 1 || (mode < 0 && Smax == 1 && 4ull * ((uint64_t)gather_cols + nhot_table) >= num_cols));
    return h;
}

// the device arrays that follow from the decisions: hot table, row blocks, the pattern plans' column values, the packed
// vector, the spread helper's column map (spread_colmap non-null), the diagonal exceptions and a split plan's planes
static int upload_plan(gl_spmv_plan p, const BlockPlan &bp, const std::vector<uint32_t> &hot_cols, std::vector<uint32_t> &ccols,
                       uint32_t gather_cols, const std::vector<uint32_t> *spread_colmap, const std::vector<uint32_t> &colbits,
                       bool diag_mode, const std::vector<float> &diag_val, const std::vector<uint32_t> &diag_has) {
    std::vector<uint4> blocks(bp.nblocks);
    for (uint32_t b = 0; b < bp.nblocks; b++) blocks[b] = make_uint4(bp.bstart[b], bp.bstart[b + 1] - bp.bstart[b], bp.seg[b], 0u);
    int rc;
    if ((rc = plan_upload(p, p->d_hot_cols, hot_cols.data(), hot_cols.size() * sizeof(uint32_t))) != GL_OK ||
        (rc = plan_upload(p, p->d_blocks, blocks.data(), blocks.size() * sizeof(uint4))) != GL_OK)
        return rc;
    if (p->pattern) {
        std::vector<uint32_t> zval(((size_t)gather_cols + 3) / 4 * 4, 0u), hval(hot_cols.size());   // value bits of the gathered / hot columns
        for (uint32_t j = 0; j < gather_cols; j++) zval[j] = colbits[p->ncompact ? ccols[j] : j];
        for (size_t j = 0; j < hot_cols.size(); j++) hval[j] = colbits[hot_cols[j]];
        if ((rc = plan_upload(p, p->d_colval, zval.data(), zval.size() * 4u)) != GL_OK ||
            (rc = plan_upload(p, p->d_hot_colval, hval.data(), hval.size() * 4u)) != GL_OK ||
            (rc = plan_alloc(p, p->d_z, ((size_t)gather_cols + 4u) * sizeof(float), (size_t)gather_cols * sizeof(float), "z")) != GL_OK)
            return rc;   // (z: whole groups of four)
        p->packed_len = (size_t)gather_cols + 4u;
    }
    if (p->ncompact) {
        while (ccols.size() % 4u) ccols.push_back(ccols.back());   // the helper kernels move four at a time
        if ((rc = plan_upload(p, p->d_ccols, ccols.data(), ccols.size() * sizeof(uint32_t))) != GL_OK) return rc;
        if (!p->pattern) {
            if ((rc = plan_alloc(p, p->d_xc, ((size_t)gather_cols + 4u) * sizeof(float), (size_t)gather_cols * sizeof(float), "xc")) != GL_OK)
                return rc;
            p->packed_len = (size_t)gather_cols + 4u;
        }
    }
    if (spread_colmap) {
        if ((rc = plan_upload(p, p->d_colmap, spread_colmap->data(), spread_colmap->size() * 4u)) != GL_OK) return rc;
        if (p->pattern && (rc = plan_upload(p, p->d_colval_bycol, colbits.data(), (size_t)p->num_cols * 4u)) != GL_OK) return rc;
    }
    if (diag_mode) {
        if ((rc = plan_upload(p, p->d_diag, diag_val.data(), diag_val.size() * sizeof(float))) != GL_OK ||
            (rc = plan_upload(p, p->d_diag_has, diag_has.data(), diag_has.size() * sizeof(uint32_t))) != GL_OK)
            return rc;
    }
    if (p->segments > 1) {
        const size_t bytes = (size_t)p->segments * (p->row_end - p->row_begin) * sizeof(float);
        if ((rc = plan_alloc(p, p->d_partials, bytes, bytes, "partials")) != GL_OK) return rc;
    }
    // the hot table's x values, gathered per run (padding slots stay 0); never null
    p->hot_x_len = p->nhot;
    return plan_alloc(p, p->d_hot_x, std::max<size_t>((size_t)p->nhot * sizeof(float), 16u), 0u, "hot_x", true);
}

// The general and pattern layouts: the plan's decisions in order.  The O(nnz) passes run on the device over a staged copy of
// the shard's CSR (gl_format.hip), or here with OpenMP (small matrices, GL_PLAN_HOST_FORMAT); the two produce identical arrays.
static int plan_general(gl_spmv_plan p, const HostCsr &a, const Knobs &k) {
    const uint32_t num_cols = a.num_cols;
    const uint64_t nnz = a.nnz;
    StagedCsr staged;
    const bool on_device = nnz > 0 && format_on_device(p->flags, nnz);
    int rc;
    if (on_device && (rc = devcsr_stage(&staged.c, a.indptr, a.indices, a.data, a.row_begin, a.row_end)) != GL_OK) return rc;

    // ---- row blocks and segments per block (gl_spmv_plan.h)
    const Shape shape = choose_shape(a.row_end - a.row_begin, num_cols, nnz, ctx().num_cus);
    const BlockPlan bp = plan_blocks(shape, a.indptr, a.row_begin, a.row_end, kMaxPlainRows);
    for (uint32_t b = 0; b < bp.nblocks; b++) p->max_plain_rows = std::max(p->max_plain_rows, bp.bstart[b + 1] - bp.bstart[b]);

    // ---- are all stored values finite?  (the SpMSpV row-wise leg multiplies every column's values by x, 0 off the frontier:
    //      only a matrix without +-inf / NaN may take it, gl_spmspv.hip)
    if (on_device) {
        int finite = 1;
        if ((rc = fmt_values_finite(staged.c, &finite)) != GL_OK) return rc;
        p->values_finite = finite != 0;
    } else {
        p->values_finite = values_finite_host(a);
    }

    // ---- pattern plan?  every column's stored values are bitwise equal (unweighted graphs, out-degree normalised PageRank
    //      matrices, bench_spmv's 1/num_rows): the stream then carries no values.  Diagonal entries are looked at separately: a
    //      matrix that is column-constant apart from its diagonal (SSSP's unit weights + zero self edges, app/sssp.h:16-62)
    //      keeps the pattern layout, the diagonal goes into a per-row array that the epilogue folds in.
    std::vector<uint32_t> colbits, diag_has;
    std::vector<float> diag_val;
    bool diag_mode = false;
    if (nnz > 0 && !(p->flags & GL_PLAN_KEEP_VALUES) && k.pattern != 0) {
        int mismatch = 0;
        uint64_t exceptions = 0;
        rc = on_device ? fmt_detect_pattern(staged.c, num_cols, colbits, diag_has, diag_val, &mismatch, &exceptions)
                       : detect_pattern_host(a, colbits, diag_has, diag_val, &mismatch, &exceptions);
        if (rc != GL_OK) return rc;
        p->pattern = !mismatch;
        diag_mode = p->pattern && exceptions > 0;
    }

    // ---- column degrees, hot columns, the self-hot rule and the packed gather vector, all recorded in one column map:
    //      per column 0x80000000 | hot slot, the packed index (0xffffffff: never gathered), or the column itself
    std::vector<uint32_t> deg, hot_cols, ccols, colmap(num_cols);
    for (uint32_t c = 0; c < num_cols; c++) colmap[c] = c;
    if (nnz > 0) {
        int bad = 0;
        rc = on_device ? fmt_column_degrees(staged.c, num_cols, deg, &bad) : column_degrees_host(a, deg, &bad);
        if (rc != GL_OK) return rc;
        if (bad) return column_error(num_cols);
        if (k.hot != 0) choose_hot_columns(k, p->flags, nnz, deg, p->max_plain_rows, bp.nblocks, p->pattern, hot_cols, colmap);
    }
    const uint32_t nhot_table = (uint32_t)((hot_cols.size() + 63) / 64 * 64);
    if (nhot_table) hot_cols.resize(nhot_table, hot_cols[0]);   // pad the table to whole wavefronts
    const bool self_hot_ok = self_hot_rule(k.helper, nnz, nhot_table);
    if (nnz > 0 && k.compact != 0 && (!self_hot_ok || k.compact == 3))
        order_packed_columns(deg, bp, bp.Smax == 1 && k.compact != 2, ccols, colmap);
    const bool compact = !ccols.empty();
    const uint32_t gather_cols = compact ? (uint32_t)ccols.size() : num_cols;

    // ---- the cold and hot entry streams (gl_spmv_plan.h)
    EmitGeneral eg;
    eg.bp = &bp;
    eg.dummy_max = gather_cols / kColdMaxDelta + 1u;   // dummies bridge gaps of > 255 columns: a unit spans at most the gather vector
    eg.colmap = colmap.data();
    eg.gather_cols = gather_cols, eg.nhot_table = nhot_table;
    eg.diag_mode = diag_mode, eg.colbits = colbits.data(), eg.diag_has = diag_has.data();
    eg.pattern = p->pattern;
    eg.group_mult = p->pattern ? kColdGroupsPattern : kColdGroupsGeneral;
    eg.hub_div = (uint32_t)std::max<long>(1, k.hub_div);
    eg.h_indptr = a.indptr, eg.num_cols = num_cols;
    std::vector<uint32_t> hub_count(bp.nblocks, 0);
    uint64_t hot_nnz = 0;
    rc = on_device ? fmt_emit_general(staged.c, eg, p, hub_count, &hot_nnz) : emit_general_host(a, eg, p, hub_count, &hot_nnz);
    if (rc != GL_OK) return rc;

    p->nblocks = bp.nblocks;
    p->segments = bp.Smax;
    p->nunits = bp.nunits;
    for (uint32_t b = 0; b < bp.nblocks; b++)
        p->max_block_rows = std::max(p->max_block_rows, bp.bstart[b + 1] - bp.bstart[b] + kHubSlots * hub_count[b]);   // LDS slots
    p->nhot = nhot_table;
    p->hot_nnz = hot_nnz;
    p->ncompact = compact ? gather_cols : 0u;
    p->mix = choose_mix(k, p->pattern, nhot_table != 0, hot_nnz, nnz);
    const Helper h = choose_helper(k.helper, self_hot_ok, p->pattern, compact, bp.Smax, gather_cols, nhot_table, num_cols);
    p->self_hot = h.self_hot;
    return upload_plan(p, bp, hot_cols, ccols, gather_cols, h.spread ? &colmap : nullptr, colbits, diag_mode, diag_val, diag_has);
}

}  // namespace gl

extern "C" {

int gl_spmv_plan_create(gl_spmv_plan *plan, uint32_t num_rows, uint32_t num_cols,
                        const uint32_t *h_indptr, const uint32_t *h_indices, const float *h_data,
                        uint32_t row_begin, uint32_t row_end) {
    return gl_spmv_plan_create_ex(plan, num_rows, num_cols, h_indptr, h_indices, h_data, row_begin, row_end, 0u);
}

int gl_spmv_plan_create_ex(gl_spmv_plan *plan, uint32_t num_rows, uint32_t num_cols,
                           const uint32_t *h_indptr, const uint32_t *h_indices, const float *h_data,
                           uint32_t row_begin, uint32_t row_end, uint32_t flags) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && h_indptr != nullptr);
    GL_ARG(row_begin <= row_end && row_end <= num_rows);
    GL_ARG(num_cols < 0x40000000u);   // (the kernels address the gathered vector by 32-bit BYTE offsets)
    const uint64_t nz0 = h_indptr[row_begin], nz1 = h_indptr[row_end];
    GL_ARG(nz1 >= nz0);
    const uint64_t nnz = nz1 - nz0;
    GL_ARG(nnz == 0 || (h_indices != nullptr && h_data != nullptr));
    for (uint32_t r = row_begin; r < row_end; r++) GL_ARG(h_indptr[r + 1] >= h_indptr[r]);

    const gl::Knobs k;
    const gl::HostCsr a{h_indptr, h_indices, h_data, num_cols, row_begin, row_end, nnz};
    gl::PlanOwner p(new gl_spmv_plan_s());
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->row_begin = row_begin;
    p->row_end = row_end;
    p->nnz = nnz;
    p->flags = flags;
    int rc;
    if (flags & GL_PLAN_REFERENCE_ORDER) {
        p->values_finite = gl::values_finite_host(a);
        rc = gl::plan_reference_order(p.get(), a);
    } else if ((flags & GL_PLAN_BOOLEAN) && nnz > 0 && gl::cdiv(num_cols, gl::kBoolPhaseCols) <= gl::kBoolMaxPhases && k.boolean != 0) {
        // (||,&&)-only plans have their own layout (gl_spmv_bool.hip); very wide matrices keep the general one
        p->values_finite = gl::values_finite_host(a);
        rc = gl::bool_plan_build(p.get(), h_indptr, h_indices, h_data);
        if (rc == GL_OK) rc = gl::bool_plan_compress(p.get());
        const long keep = gl::debug_knob("bool_keep", -1);
        p->bool_keep = (keep == 0 || keep == 1) ? (int8_t)keep : (int8_t)-1;
    } else {
        rc = gl::plan_general(p.get(), a, k);
    }
    if (rc != GL_OK) return rc;
    *plan = p.release();
    return GL_OK;
}

int gl_spmv_plan_destroy(gl_spmv_plan p) {
    if (!p) return GL_OK;
    gl::spmspv_detach_everywhere(p);   // attachments do not own the plan; none may outlive it
    (void)hipFree(p->d_entries);
    (void)hipFree(p->d_bases);
    (void)hipFree(p->d_units);
    (void)hipFree(p->d_hub_rows);
    (void)hipFree(p->d_hot);
    (void)hipFree(p->d_hot_hdr);
    (void)hipFree(p->d_present);
    (void)hipFree(p->d_hot_cols);
    (void)hipFree(p->d_hot_x);
    (void)hipFree(p->d_spans);
    (void)hipFree(p->d_blocks);
    (void)hipFree(p->d_colval);
    (void)hipFree(p->d_hot_colval);
    (void)hipFree(p->d_ccols);
    (void)hipFree(p->d_colmap);
    (void)hipFree(p->d_packed_twin);
    (void)hipFree(p->d_hot_x_twin);
    (void)hipFree(p->d_colval_bycol);
    (void)hipFree(p->d_xc);
    (void)hipFree(p->d_diag);
    (void)hipFree(p->d_diag_has);
    (void)hipFree(p->d_z);
    (void)hipFree(p->d_partials);
    (void)hipFree(p->d_xbits);
    (void)hipFree(p->d_csr_indptr);
    (void)hipFree(p->d_csr_indices);
    (void)hipFree(p->d_parents_scratch);
    (void)hipFree(p->d_cc_scratch);
    (void)hipFree(p->d_tc_scratch);
    (void)hipFree(p->d_kcore_scratch);
    (void)hipFree(p->d_color_scratch);
    (void)hipFree(p->d_truss_scratch);
    (void)hipFree(p->d_msf_scratch);
    (void)hipFree(p->d_match_scratch);
    (void)hipFree(p->d_lpa_scratch);
    (void)hipFree(p->d_louvain_scratch);
    (void)hipFree(p->d_scc_scratch);
    (void)hipFree(p->d_bicc_scratch);
    (void)hipFree(p->d_topo_scratch);
    (void)hipFree(p->d_msbfs_scratch);
    (void)hipFree(p->d_sim_scratch);
    (void)hipFree(p->d_bc_scratch);
    if (p->h_bc_pinned) (void)hipHostFree(p->h_bc_pinned);
    (void)hipFree(p->d_csr_data);
    delete p;
    return GL_OK;
}

int gl_spmv_plan_describe(gl_spmv_plan p, gl_spmv_plan_desc *out) {
    GL_ARG(p != nullptr && out != nullptr);
    out->nnz = p->nnz;
    out->device_bytes = p->device_bytes;
    out->groups = p->ngroups;
    out->hot_nnz = p->hot_nnz;
    out->num_units = p->nunits;
    out->blocks = p->nblocks;
    out->segments = p->segments;
    out->max_block_rows = p->max_block_rows;
    out->hot_columns = p->nhot;
    out->packed_columns = p->ncompact;
    out->layout = p->reference_order ? GL_LAYOUT_REFERENCE_ORDER : p->boolean ? GL_LAYOUT_BOOLEAN : (p->pattern ? GL_LAYOUT_PATTERN : GL_LAYOUT_GENERAL);
    out->mix = p->mix;
    out->helper = p->boolean ? GL_HELPER_NONE : p->self_hot ? GL_HELPER_SELF_HOT : p->d_colmap ? GL_HELPER_SPREAD
                  : (p->pattern || p->nhot || p->ncompact) ? GL_HELPER_GATHER : GL_HELPER_NONE;
    return GL_OK;
}

int gl_spmv_plan_values_finite(gl_spmv_plan p, int *finite) {
    GL_ARG(p != nullptr && finite != nullptr);
    *finite = p->values_finite ? 1 : 0;
    return GL_OK;
}

int gl_spmv_plan_export(gl_spmv_plan p, int array, void *h_dst, size_t capacity, size_t *bytes) {
    GL_REQUIRE_INIT();
    GL_ARG(p != nullptr && bytes != nullptr);
    const void *src = nullptr;
    size_t n = 0;
    switch (array) {
        case GL_PLAN_ARRAY_ENTRIES: src = p->d_entries, n = p->b_entries; break;
        case GL_PLAN_ARRAY_BASES: src = p->d_bases, n = p->b_bases; break;
        case GL_PLAN_ARRAY_UNITS: src = p->d_units, n = p->b_units; break;
        case GL_PLAN_ARRAY_HUB_ROWS: src = p->d_hub_rows, n = p->b_hub_rows; break;
        case GL_PLAN_ARRAY_SPANS: src = p->d_spans, n = p->b_spans; break;
        case GL_PLAN_ARRAY_HOT: src = p->d_hot, n = p->b_hot; break;
        case GL_PLAN_ARRAY_HOT_HDR: src = p->d_hot_hdr, n = p->b_hot_hdr; break;
        case GL_PLAN_ARRAY_PRESENT: src = p->d_present, n = p->b_present; break;
        default: return gl::set_error(GL_ERR_INVALID_ARG, "gl_spmv_plan_export: unknown array %d", array);
    }
    *bytes = n;
    if (!h_dst) return GL_OK;
    GL_ARG(capacity >= n);
    if (n) {
        GL_HIP(hipStreamSynchronize(gl::ctx().stream));
        GL_HIP(hipMemcpy(h_dst, src, n, hipMemcpyDeviceToHost));
    }
    return GL_OK;
}

}  // extern "C"
