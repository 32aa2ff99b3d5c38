// Label propagation communities (gl_lpa): Raghavan, Albert & Kumara's label propagation in Cordasco & Gargano's semi-synchronous
// form over the plain CSR copy that every GL_PLAN_BOOLEAN plan keeps (gl_rows.h), on a square, whole-matrix plan whose
// rows are strictly ascending sets N(v) and whose pattern is SYMMETRIC, over n = num_rows vertices.  An entry (v, v) is ignored.
//
//   label[v]   starts as init[v] (no init: v).  EVALUATING a vertex v with a neighbour: cnt(l) = neighbours carrying l, best = max
//              cnt, cur = cnt(label[v]); if best > cur, label[v] becomes the SMALLEST l with cnt(l) == best, otherwise it stays
//   colour classes (d_color, a proper colouring): a sweep evaluates class 0, then class 1, ... in place, ONE LAUNCH PER CLASS: no
//              two vertices of a launch are adjacent, so the result is the sequential loop in (colour, vertex) order
//   synchronous (no d_color): a sweep evaluates every vertex from the previous sweep's labels, into the other of two buffers
//   the run ends after the first sweep that changes nothing (converged) or after max_sweeps sweeps
//
// STATE: the labels; one FLAG word per vertex -- kLpaLinked: v has a neighbour (set once), kLpaActive: a neighbour
// changed since v's last evaluation (sweep 1: every linked vertex) --; the vertices bucketed by colour (histogram, scan, scatter:
// list and offs); a CONTROL RECORD {done, sweeps, converged, which} + the words launches add to (a line of their own).
//   class  over the slice [offs[c], offs[c + 1]) of the list, a thread per listed vertex: a vertex whose flag says active is
//          evaluated and its active bit cleared -- by its own thread, the only one that clears it; a vertex that changes sets the
//          flag of every neighbour to linked | active
//   turn   (one thread) sweeps += 1; a sweep without a change ends the run: converged, done; so does sweep max_sweeps
// THE MODE OF A ROW, exact in three regimes:
//   a thread    rows of at most lpa_cut <= 8 entries: eight index loads, then eight label gathers in flight, counted in registers
//   a wavefront every longer row, 256 entries per step (rows_walk_wave: the four gathers behind the four index loads), counted in
//               the wavefront's own LDS table of (label, count) slots, claimed with an LDS compare-and-swap within 16 probes and
//               counted with an LDS add.  lpa_table = 2048 slots: 16 KiB per wavefront, 64 KiB per workgroup (the most a launch
//               gets without asking), so the 160 KiB of a compute unit hold 2 workgroups = 8 of its 32 wavefront slots.  512
//               slots keep all 32 and were 1.8 - 2.6 times SLOWER, 1024 slots 1.3 - 1.7 times (EXPERIMENTS.md Round 23): the
//               hubs' partition passes, one wavefront each, are the critical path of a class launch, and half the passes beat
//               four times the occupancy.  best
//               and the smallest label are ONE max-reduction of count << 32 | ~label over the slots, cur a look-up
//   partitions  a label that finds no slot within its probes: the row is counted again in `parts` passes, pass p taking the labels
//               whose hash (bits apart from the slot's) says p; best is the maximum over the passes, cur comes from the pass of
//               the vertex's own label.  An overflowing pass restarts the row with 4 x parts; in sweep 1, where a hub's labels
//               are mostly distinct, the first restart jumps to a table half full at most.  Exact whatever the table's size; a hub of d
//               entries with k distinct labels costs about k / (table / 2) passes over its row.  (A global scratch table was
//               not built.)
// MEMORY RULE and GATING: gl_rounds.h.  Within a class launch no label that is read is written (colour classes: the neighbours of
// a class's vertices are in other classes; synchronous: the other buffer), so labels are plain loads and stores.  Atomic-only
// inside a class launch: the flags that a changing vertex sets (several workgroups may store the same word, all the same value;
// nobody reads it in this launch: the owner of that word is in another class, or reads the other flag array) and the record's
// second line.  A vertex's own flag is read and cleared by its own thread.  The host enqueues lpa_batch sweeps of (classes + 1)
// launches blindly; every launch returns at once when the record says done.  At most max_sweeps sweeps run.
#include "gl_classes.h"
#include "graphlily_hip_lpa.h"

namespace gl {

// the control record (words); the second 128-byte line holds what init, check and class launches add to (gl_classes.h names the
// three words of the colour bucketing)
enum : uint32_t { kLpaDone = 0, kLpaSweeps = 1, kLpaConverged = 2, kLpaWhich = 3, kLpaRecordWords = 4, kLpaSweepChanges = 32,
                  kLpaChanges = 34, kLpaEvals = 36, kLpaBadInit = 38, kLpaStuck = 41, kLpaReadEnd = 42 };
constexpr uint32_t kLpaActive = 1u, kLpaLinked = 2u;
constexpr uint32_t kLpaThreadMax = 8;            // entries a thread counts in registers, at most

// label[v] = init[v] or v, the flags (none for a plan without entries); a label 0xffffffff is counted
__global__ __launch_bounds__(256) void lpa_init_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                       const uint32_t *init, uint32_t n, uint32_t nz_base, uint32_t *label,
                                                       uint32_t *__restrict__ flags_a, uint32_t *__restrict__ flags_b, uint32_t *ctl) {
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < n; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        const uint32_t l = init ? init[v] : v;
        if (l == kLpaEmpty) ga_add(ctl + kLpaBadInit, 1u);
        label[v] = l;
        if (row_ptr == nullptr) continue;
        const uint32_t beg = row_ptr[v] - nz_base, end = row_ptr[v + 1u] - nz_base;
        const bool linked = end - beg > 1u || (end - beg == 1u && row_idx[beg] != v);
        flags_a[v] = linked ? (kLpaLinked | kLpaActive) : 0u;
        flags_b[v] = linked ? kLpaLinked : 0u;
    }
}

struct LpaArgs {
    const uint32_t *row_ptr, *row_idx, *list, *offs;              // list == nullptr: synchronous, one class of all vertices
    uint32_t *label[2], *flags[2], *ctl;
    uint32_t n, nz_base, cut, table_mask, use_active;
};

// One pass of the wavefront over the row [b, e) of vertex `row`: counts the neighbours' labels of partition `part` (of parts_mask
// + 1) in the table and folds the partition's best count << 32 | ~label into `best`, and the count of `own` into `cur` if `own`
// belongs to the partition.  -> true (in every lane) when a label found no slot: the table then says nothing.
__device__ __forceinline__ bool lpa_count_pass(const LpaArgs &a, const uint32_t *src, uint32_t *keys, uint32_t *cnt, uint32_t b, uint32_t e,
                                               uint32_t lane, uint32_t row, uint32_t own, uint32_t parts_mask, uint32_t part,
                                               unsigned long long &best, uint32_t &cur) {
    const uint32_t mask = a.table_mask, probes = min(kLpaProbes, mask + 1u);
    for (uint32_t s = lane; s <= mask; s += 64u) {
        keys[s] = kLpaEmpty;
        cnt[s] = 0u;
    }
    lpa_wave_sync();
    bool fail = false;
    rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
        uint32_t l[4];
#pragma unroll
        for (int u = 0; u < 4; u++) l[u] = (c[u] < a.n && c[u] != row) ? src[c[u]] : kLpaEmpty;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (l[u] == kLpaEmpty) continue;
            const uint32_t m = lpa_mix(l[u]);
            if (((m >> 12) & parts_mask) != part) continue;
            uint32_t h = m & mask;
            bool placed = false;
            for (uint32_t i = 0; i < probes; i++) {
                const uint32_t k = atomicCAS(&keys[h], kLpaEmpty, l[u]);
                if (k == kLpaEmpty || k == l[u]) {
                    atomicAdd(&cnt[h], 1u);
                    placed = true;
                    break;
                }
                h = (h + 1u) & mask;
            }
            fail |= !placed;
        }
        return __any(fail) != 0;
    });
    lpa_wave_sync();
    if (__any(fail)) return true;
    unsigned long long cand = 0ull;
    for (uint32_t s = lane; s <= mask; s += 64u) {
        const uint32_t k = keys[s];
        if (k != kLpaEmpty) {
            const unsigned long long x = ((unsigned long long)cnt[s] << 32) | (uint32_t)~k;
            cand = x > cand ? x : cand;
        }
    }
    cand = lpa_wave_max(cand);
    best = cand > best ? cand : best;
    const uint32_t m = lpa_mix(own);
    if (((m >> 12) & parts_mask) == part) {                       // (uniform: every lane looks the same slots up)
        uint32_t h = m & mask;
        for (uint32_t i = 0; i < probes; i++) {
            const uint32_t k = keys[h];
            if (k == own) cur = cnt[h];
            if (k == own || k == kLpaEmpty) break;
            h = (h + 1u) & mask;
        }
    }
    lpa_wave_sync();                                              // (the next pass clears the table)
    return false;
}

extern __shared__ uint32_t lpa_tables[];                          // per wavefront: table_mask + 1 keys, then as many counts

__global__ __launch_bounds__(256) void lpa_class_kernel(LpaArgs a, uint32_t cls) {
    if (a.ctl[kLpaDone] != 0u) return;
    const bool sync = a.list == nullptr;
    const uint32_t lo = sync ? 0u : a.offs[cls], hi = sync ? a.n : a.offs[cls + 1u];
    const uint32_t which = sync ? (a.ctl[kLpaWhich] & 1u) : 0u;
    const uint32_t *src = a.label[which];
    uint32_t *dst = a.label[sync ? which ^ 1u : 0u];
    uint32_t *mine = a.flags[which], *theirs = a.flags[sync ? which ^ 1u : 0u];
    const bool first_sweep = a.ctl[kLpaSweeps] == 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *keys = lpa_tables + (size_t)wave * 2u * (a.table_mask + 1u), *cnt = keys + (a.table_mask + 1u);
    const uint32_t count = hi - lo, nwaves = gridDim.x * 4u;
    // listed vertices per wavefront: 64, fewer when the slice is shorter than the launch (as color_round_kernel)
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t nwords = (uint32_t)(((uint64_t)count + per - 1u) / per);
    uint32_t evals = 0, changes = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t item = (uint64_t)wd * per + lane;
        const bool in = lane < per && item < count;
        uint32_t v = 0, beg = 0, end = 0, own = 0, fresh = 0;
        bool evaluate = false;
        if (in) {
            v = sync ? (uint32_t)item : a.list[lo + item];
            const uint32_t flag = mine[v];
            evaluate = (flag & (a.use_active ? kLpaActive : kLpaLinked)) != 0u;
            own = fresh = src[v];
            if (evaluate) {
                mine[v] = kLpaLinked;                             // (only linked vertices are ever evaluated)
                beg = a.row_ptr[v] - a.nz_base;
                end = a.row_ptr[v + 1u] - a.nz_base;
                evals += 1u;
            }
        }
        if (evaluate && end - beg <= a.cut) {                     // a thread's row: cut <= kLpaThreadMax entries, in registers
            uint32_t c[kLpaThreadMax], l[kLpaThreadMax];
#pragma unroll
            for (uint32_t u = 0; u < kLpaThreadMax; u++) c[u] = end - beg > u ? a.row_idx[beg + u] : kLpaEmpty;
#pragma unroll
            for (uint32_t u = 0; u < kLpaThreadMax; u++) {
                c[u] = (c[u] < a.n && c[u] != v) ? c[u] : kLpaEmpty;
                l[u] = c[u] != kLpaEmpty ? src[c[u]] : kLpaEmpty;
            }
            unsigned long long best = 0ull;
            uint32_t cur = 0;
#pragma unroll
            for (uint32_t i = 0; i < kLpaThreadMax; i++) {
                uint32_t k = 0;
#pragma unroll
                for (uint32_t j = 0; j < kLpaThreadMax; j++) k += l[j] == l[i] ? 1u : 0u;
                const unsigned long long x = l[i] != kLpaEmpty ? ((unsigned long long)k << 32) | (uint32_t)~l[i] : 0ull;
                best = x > best ? x : best;
                cur += l[i] == own ? 1u : 0u;
            }
            if ((uint32_t)(best >> 32) > cur) {
                fresh = ~(uint32_t)best;
                changes += 1u;
#pragma unroll
                for (uint32_t u = 0; u < kLpaThreadMax; u++)
                    if (c[u] != kLpaEmpty) ga_store(theirs + c[u], kLpaLinked | kLpaActive);
            }
            beg = end;
        }
        rows_walk_takeover(beg, end, [&](int srcl, uint32_t b, uint32_t e) {
            const uint32_t row = __shfl(v, srcl), mylabel = __shfl(own, srcl);
            unsigned long long best = 0ull;
            uint32_t cur = 0;
            bool stuck = false;
            for (uint32_t parts = 1u;;) {
                best = 0ull;
                cur = 0u;
                bool overflow = false;
                for (uint32_t part = 0; part < parts && !overflow; part++)
                    overflow = lpa_count_pass(a, src, keys, cnt, b, e, lane, row, mylabel, parts - 1u, part, best, cur);
                if (!overflow) break;
                if (parts >= kLpaMaxParts) {
                    stuck = true;
                    break;
                }
                // sweep 1: a hub's labels are mostly distinct -- straight to tables half full at most; later: four times as many
                uint32_t jump = 1u;
                if (first_sweep)
                    while (jump < kLpaMaxParts && (uint64_t)jump * (a.table_mask + 1u) < 2ull * (e - b)) jump <<= 1;
                parts = min(kLpaMaxParts, max(parts * 4u, jump));
            }
            if (stuck) {
                if (lane == 0u) ga_store(a.ctl + kLpaStuck, 1u);
                return;
            }
            if ((uint32_t)(best >> 32) > cur) {                   // (uniform: every lane holds the same best and cur)
                rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (c[u] < a.n && c[u] != row) ga_store(theirs + c[u], kLpaLinked | kLpaActive);
                    return false;
                });
                if ((int)lane == srcl) {
                    fresh = ~(uint32_t)best;
                    changes += 1u;
                }
            }
        });
        if (in && (sync || fresh != own)) dst[v] = fresh;
    }
    evals = lpa_wave_sum(evals);
    changes = lpa_wave_sum(changes);
    if (lane == 0u) {
        if (evals != 0u) ga_add(reinterpret_cast<unsigned long long *>(a.ctl + kLpaEvals), (unsigned long long)evals);
        if (changes != 0u) ga_add(a.ctl + kLpaSweepChanges, changes);
    }
}

// behind the last class of a sweep: plain loads and stores, a launch of its own
__global__ void lpa_turn_kernel(uint32_t *ctl, uint32_t max_sweeps, uint32_t sync) {
    if (threadIdx.x != 0u || blockIdx.x != 0u || ctl[kLpaDone] != 0u) return;
    const uint32_t changed = ctl[kLpaSweepChanges];
    ctl[kLpaSweepChanges] = 0u;
    *reinterpret_cast<unsigned long long *>(ctl + kLpaChanges) += changed;
    const uint32_t sweeps = ctl[kLpaSweeps] + 1u;
    ctl[kLpaSweeps] = sweeps;
    if (sync) ctl[kLpaWhich] ^= 1u;                               // the labels just written are the next sweep's source
    if (changed == 0u) ctl[kLpaConverged] = ctl[kLpaDone] = 1u;
    else if (sweeps >= max_sweeps) ctl[kLpaDone] = 1u;
}

// the words of the plan's scratch behind the control record: two flag arrays, the second label buffer, the class list, the
// histogram (then the scatter's cursors) of n words each, and n + 1 class offsets
constexpr size_t lpa_scratch_bytes(size_t n) { return kRoundsCtlBytes + 4u * (6u * n + 1u); }

static int lpa(gl_spmv_plan p, const uint32_t *d_color, const uint32_t *d_init, uint32_t *d_label, uint32_t max_sweeps, uint64_t *h_stats,
               const char *who) {
    int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_simple");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    if (h_stats) {
        h_stats[0] = h_stats[4] = 1u;
        h_stats[1] = h_stats[2] = h_stats[3] = 0u;
    }
    if (n == 0u) return GL_OK;
    rc = plan_scratch(p->d_lpa_scratch, lpa_scratch_bytes(n), who, "control record, flags, labels, class list, histogram and offsets");
    if (rc != GL_OK) return rc;
    uint32_t *ctl = reinterpret_cast<uint32_t *>(p->d_lpa_scratch);
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    static_assert((kLpaRecordWords + kLpaReadEnd - kLpaTop) * 4u <= 64u, "the record fits the page-locked staging words");
    const auto copy_record = [&] {
        const hipError_t e = hipMemcpyAsync(w, ctl, kLpaRecordWords * 4u, hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipMemcpyAsync(w + kLpaRecordWords, ctl + kLpaTop, (kLpaReadEnd - kLpaTop) * 4u, hipMemcpyDeviceToHost, s);
    };
    const auto word = [&](uint32_t k) { return w[kLpaRecordWords + k - kLpaTop]; };      // a word of the second line, as read back
    const unsigned vertex_grid = rows_stream_grid(n);
    LpaArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.ctl = ctl;
    a.flags[0] = ctl + kRoundsCtlBytes / 4u;
    a.flags[1] = a.flags[0] + n;
    a.label[0] = d_label;
    a.label[1] = a.flags[1] + n;
    uint32_t *list = a.label[1] + n, *hist = list + n, *offs = hist + n;
    a.list = d_color ? list : nullptr;
    a.offs = offs;
    a.n = n;
    a.nz_base = p->csr_nz_base;
    const bool empty = p->nnz == 0;
    GL_HIP(hipMemsetAsync(ctl, 0, kRoundsCtlBytes, s));
    lpa_init_kernel<<<vertex_grid, 256, 0, s>>>(empty ? nullptr : a.row_ptr, a.row_idx, d_init, n, a.nz_base, d_label, a.flags[0], a.flags[1], ctl);
    uint64_t launches = 1;
    if (d_color && !empty) {                                      // the classes: histogram (with the check), scan, scatter
        GL_HIP(hipMemsetAsync(hist, 0, 4u * (size_t)n, s));
        lpa_check_kernel<<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, d_color, n, a.nz_base, hist, ctl);
        lpa_scan_kernel<<<1, 1024, 0, s>>>(hist, offs, ctl, n);
        lpa_scatter_kernel<<<vertex_grid, 256, 0, s>>>(d_color, n, hist, list);
        launches += 3;
    }
    GL_LAUNCH_CHECK();
    GL_HIP(copy_record());
    GL_HIP(hipStreamSynchronize(s));
    if (word(kLpaBadInit) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: %u words of d_init hold the label 0xffffffff, which is reserved as the empty key of the "
                         "label tables (d_label is then written, and not a result)", who, word(kLpaBadInit));
    if (word(kLpaBadColor) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: %u words of d_color hold a colour >= n = %u (d_label is then written, and not a result)", who,
                         word(kLpaBadColor), n);
    if (word(kLpaImproper) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: d_color is not a proper colouring: %u entries (v, u) have colour[v] == colour[u], so two "
                         "vertices of one class launch would read and write each other's labels (gl_color gives a proper one; d_label is "
                         "then written, and not a result)", who, word(kLpaImproper));
    if (empty) {                                                  // no entries: nobody has a neighbour, the first sweep is empty
        if (h_stats) h_stats[3] = launches;
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 23): lpa_cut = entries of a row that a thread counts in
    // registers (0 .. 8; longer rows go to the wavefront), lpa_grid = workgroups per compute unit of a class launch, lpa_batch =
    // sweeps enqueued between two read-backs of the control record, lpa_table = slots of a wavefront's LDS table (a power of two,
    // 8 .. 2048; the header says why 2048), lpa_active = 0 evaluates every linked vertex in every sweep
    const uint32_t classes = d_color ? word(kLpaTop) + 1u : 1u;
    const RowsWalkShape shape = rows_walk_shape(n, 0, 0, debug_knob("lpa_grid", 8));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("lpa_batch", 4), 64));
    uint32_t table = 8;
    while (table < 2048u && (long)table < debug_knob("lpa_table", 2048)) table <<= 1;
    a.cut = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("lpa_cut", kLpaThreadMax), kLpaThreadMax));
    a.table_mask = table - 1u;
    a.use_active = debug_knob("lpa_active", 1) != 0 ? 1u : 0u;
    const size_t lds = 4u * 2u * (size_t)table * sizeof(uint32_t);      // four wavefronts' keys and counts: 64 KiB at most
    const uint32_t sync = d_color ? 0u : 1u;
    rc = rounds_run(
        batch, (uint64_t)max_sweeps + batch, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                for (uint32_t c = 0; c < classes; c++) lpa_class_kernel<<<shape.grid, 256, lds, s>>>(a, c);
                lpa_turn_kernel<<<1, 64, 0, s>>>(ctl, max_sweeps, sync);
            }
            return (uint64_t)batch * ((uint64_t)classes + 1u);
        },
        copy_record,
        [&] { return word(kLpaStuck) != 0u ? kRoundsStuck : w[kLpaDone] != 0u ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t sweeps) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu sweeps of %u allowed on %u vertices (%u sweeps counted%s)", who,
                             (unsigned long long)sweeps, max_sweeps, n, w[kLpaSweeps],
                             word(kLpaStuck) ? "; a row's labels did not fit the table in 2^20 partitions" : "");
        });
    if (rc != GL_OK) return rc;
    if (w[kLpaWhich] & 1u) {                                      // synchronous, an odd number of sweeps: the result is in the scratch buffer
        GL_HIP(hipMemcpyAsync(d_label, a.label[1], 4u * (size_t)n, hipMemcpyDeviceToDevice, s));
        GL_HIP(hipStreamSynchronize(s));
    }
    if (h_stats) {
        h_stats[0] = w[kLpaSweeps];
        h_stats[1] = (uint64_t)word(kLpaChanges) | ((uint64_t)word(kLpaChanges + 1u) << 32);
        h_stats[2] = (uint64_t)word(kLpaEvals) | ((uint64_t)word(kLpaEvals + 1u) << 32);
        h_stats[3] = launches;
        h_stats[4] = w[kLpaConverged];
    }
    return GL_OK;
}

}  // namespace gl

int gl_lpa(gl_spmv_plan plan, const uint32_t *d_color, const uint32_t *d_init, uint32_t *d_label, uint32_t max_sweeps, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_label != nullptr);
    GL_ARG(max_sweeps != 0u);
    GL_ARG(d_color != d_label);
    return gl::lpa(plan, d_color, d_init, d_label, max_sweeps, h_stats, "gl_lpa");
}
