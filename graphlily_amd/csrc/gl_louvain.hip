// Louvain local moving (gl_louvain_move): one level of Blondel et al.'s modularity optimisation in the colour-class form of Lu,
// Halappanavar & Kalyanaraman over the plain CSR copy that every GL_PLAN_BOOLEAN plan keeps (gl_rows.h), on a square,
// whole-matrix plan whose rows are strictly ascending sets N(v) and whose pattern is SYMMETRIC, over n = num_rows vertices, with a
// weight per entry of the copy and a weight k[v] per vertex.  An entry (v, v) is ignored.  graphlily_hip_louvain.h states the rule.
//
// STATE: the labels (the caller's array); k[v]; tot[c]; the vertices bucketed by colour (gl_classes.h: list and
// offs); a MOVER LIST of (vertex, new label) pairs; a CONTROL RECORD -- first line {done, sweeps, reason, stuck, q_first, q_last,
// moves, evaluations, two_m}, which only one-thread launches write; second line: what the launches between them add to.
//   class  over the slice [offs[c], offs[c + 1]) of the list, a thread per listed vertex: a vertex with a neighbour is evaluated
//          from label, k and tot AS THEY STAND -- nothing that the launch reads is written by it; a vertex that moves is appended
//          to the mover list (one ballot and one atomic add per wavefront)
//   apply  over the mover list: label[v] = new, tot[old] -= k[v], tot[new] += k[v] (integer adds: they commute); one thread adds
//          the list's length to the sweep's moves and empties the OTHER of the two tails, which the next class launch appends to
//   q      (behind a sweep's last apply) one pass over the rows and over tot: In and the sum of tot^2, 64-bit integer adds
//   turn   (one thread) Q = two_m * In - sum tot^2; sweeps += 1; the three stop rules
// THE BEST COMMUNITY OF A ROW, exact in gl_lpa's three regimes:
//   a thread    rows of at most louvain_cut <= 8 entries: indices, weights, labels and tot gathers in flight, summed in registers
//   a wavefront every longer row, 256 entries per step, summed in the wavefront's own LDS table of (label, weight sum) slots,
//               claimed with an LDS compare-and-swap within 16 probes and summed with an LDS add; every occupied slot then
//               gathers tot[label] once and gives a signed 64-bit score; the largest score, then the smallest label carrying it:
//               two wavefront reductions.  louvain_table = 2048 slots as gl_lpa's (16 KiB per wavefront, 64 KiB per workgroup)
//   partitions  a label that finds no slot: the row is summed again in `parts` passes by the labels' hash, as gl_lpa; (score,
//               label) is compared across the passes, kin(own) comes from the pass of the vertex's own label
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only inside a launch: the mover tail and the record's second line (class), tot
// (apply; nobody reads it there).  The host enqueues louvain_batch sweeps of (2 classes + 2) launches blindly; every launch returns
// at once when the record says done.  At most max_sweeps sweeps run.
#include "gl_classes.h"
#include "graphlily_hip_louvain.h"

namespace gl {

// the control record (words; 64-bit values on even words); gl_classes.h names the three words of the colour bucketing
enum : uint32_t { kLvDone = 0, kLvSweeps = 1, kLvReason = 2, kLvStuckSeen = 3, kLvQFirst = 4, kLvQLast = 6, kLvMoves = 8, kLvEvals = 10,
                  kLvTwoM = 12, kLvRecordWords = 14, kLvSweepMoves = 32, kLvTail = 34, kLvSweepEvals = 36, kLvBadWeight = 38, kLvStuck = 41,
                  kLvBadK = 42, kLvSumK = 44, kLvReadEnd = 46, kLvIn = 46, kLvSq = 48 };
constexpr uint32_t kLvThreadMax = 8;             // entries a thread sums in registers, at most
constexpr long long kLvNoScore = (long long)(1ull << 63);      // below every score: |score| < 2^62

__device__ __forceinline__ unsigned long long *lv_u64(uint32_t *ctl, uint32_t word) { return reinterpret_cast<unsigned long long *>(ctl + word); }

__device__ __forceinline__ unsigned long long louvain_wave_sum64(unsigned long long x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += __shfl_xor(x, d);
    return x;
}

__device__ __forceinline__ uint32_t louvain_wave_min(uint32_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = min(x, (uint32_t)__shfl_xor(x, d));
    return x;
}

// One pass over the rows, a thread per row and the wavefront for the rows above kLpaCheckCut entries.
// kInit: k[v] = vweight[v] or the sum of v's entry weights, tot[v] = k[v], label[v] = v; counted: zero weights, k[v] below the
//        sum, the sum of all k.
// else:  In += k[v] - (the weights of v's entries whose other end carries another label), Sq += tot[v]^2.
template <bool kInit>
__global__ __launch_bounds__(256) void louvain_rows_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                           const uint32_t *__restrict__ weight, const uint32_t *__restrict__ vweight, uint32_t n,
                                                           uint32_t nz_base, uint32_t *label, uint32_t *k, uint32_t *tot, uint32_t *ctl) {
    if (!kInit && ctl[kLvDone] != 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long acc_a = 0, acc_b = 0;
    uint32_t zero = 0, badk = 0;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        const bool in = v64 < n;
        uint32_t beg = 0, end = 0, lv = 0;
        if (in) {
            beg = row_ptr[v] - nz_base;
            end = row_ptr[v + 1u] - nz_base;
            if (!kInit) lv = label[v];
        }
        unsigned long long sum = 0;
        if (end - beg <= kLpaCheckCut) {
            for (; beg < end; beg++) {
                const uint32_t u = row_idx[beg];
                if (u >= n || u == v) continue;
                const uint32_t w = weight ? weight[beg] : 1u;
                if (kInit) {
                    sum += w;
                    zero += w == 0u ? 1u : 0u;
                } else if (label[u] != lv) {
                    sum += w;
                }
            }
        }
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t row = __shfl(v, src), rl = __shfl(lv, src);
            unsigned long long part = 0;
            rows_walk_wave(row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (c[u] >= n || c[u] == row) continue;       // (a column below n: the position is inside the row)
                    const uint32_t w = weight ? weight[base + 64u * u + lane] : 1u;
                    if (kInit) {
                        part += w;
                        zero += w == 0u ? 1u : 0u;
                    } else if (label[c[u]] != rl) {
                        part += w;
                    }
                }
                return false;
            });
            part = louvain_wave_sum64(part);
            if ((int)lane == src) sum = part;
        });
        if (!in) continue;
        if (kInit) {
            uint32_t kv = (uint32_t)min(sum, 0xffffffffull);
            if (vweight) {
                kv = vweight[v];
                if (kv < sum) badk += 1u;
            }
            k[v] = kv;
            tot[v] = kv;
            label[v] = v;
            acc_a += vweight ? (unsigned long long)kv : sum;
        } else {
            const unsigned long long t = tot[v];
            acc_a += (unsigned long long)k[v] - sum;
            acc_b += t * t;
        }
    }
    acc_a = louvain_wave_sum64(acc_a);
    acc_b = louvain_wave_sum64(acc_b);
    zero = lpa_wave_sum(zero);
    badk = lpa_wave_sum(badk);
    if (lane == 0u) {
        if (acc_a != 0ull) ga_add(lv_u64(ctl, kInit ? kLvSumK : kLvIn), acc_a);
        if (acc_b != 0ull) ga_add(lv_u64(ctl, kLvSq), acc_b);
        if (zero != 0u) ga_add(ctl + kLvBadWeight, zero);
        if (badk != 0u) ga_add(ctl + kLvBadK, badk);
    }
}

// A sum that the launches before this one added to, read and emptied by the one thread of a turn.  Through the atomic wrappers:
// as plain code the read became a scalar load and the reset a vector store to the same word, which the hardware does not order,
// and the read returned the zero.
__device__ __forceinline__ unsigned long long louvain_take(unsigned long long *p) {
    const unsigned long long x = ga_load(p);
    ga_store(p, 0ull);
    return x;
}
__device__ __forceinline__ uint32_t louvain_take(uint32_t *p) {
    const uint32_t x = ga_load(p);
    ga_store(p, 0u);
    return x;
}

// Q of the labels as they stand, from the sums a q launch left (which are emptied)
__device__ __forceinline__ long long louvain_take_q(uint32_t *ctl, unsigned long long two_m) {
    const unsigned long long in = louvain_take(lv_u64(ctl, kLvIn)), sq = louvain_take(lv_u64(ctl, kLvSq));
    return (long long)(two_m * in - sq);
}

// behind the init and the first q launch: two_m and the singletons' Q
__global__ void louvain_begin_kernel(uint32_t *ctl) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    const unsigned long long two_m = ga_load(lv_u64(ctl, kLvSumK));
    *lv_u64(ctl, kLvTwoM) = two_m;
    const long long q = louvain_take_q(ctl, two_m);
    *lv_u64(ctl, kLvQFirst) = (unsigned long long)q;
    *lv_u64(ctl, kLvQLast) = (unsigned long long)q;
}

struct LouvainArgs {
    const uint32_t *row_ptr, *row_idx, *weight, *list, *offs;
    uint32_t *label, *k, *tot, *movers, *ctl;
    uint32_t n, nz_base, cut, table_mask;
};

// (score, label) a replaces b: the larger score, then the smaller label
__device__ __forceinline__ bool louvain_better(long long sa, uint32_t la, long long sb, uint32_t lb) { return sa > sb || (sa == sb && la < lb); }

// One pass of the wavefront over the row [b, e) of vertex `row`: sums the weights towards the neighbours' labels of partition
// `part` (of parts_mask + 1) in the table, folds the partition's best (score, label) over the labels other than `own` into
// (best, bl), and the sum of `own` into kin_own if `own` belongs to the partition.  -> true (in every lane) when a label found no
// slot: the table then says nothing.
__device__ __forceinline__ bool louvain_sum_pass(const LouvainArgs &a, uint32_t *keys, uint32_t *sums, uint32_t b, uint32_t e, uint32_t lane,
                                                 uint32_t row, uint32_t own, long long two_m, long long kv, uint32_t parts_mask, uint32_t part,
                                                 long long &best, uint32_t &bl, uint32_t &kin_own) {
    const uint32_t mask = a.table_mask, probes = min(kLpaProbes, mask + 1u);
    for (uint32_t s = lane; s <= mask; s += 64u) {
        keys[s] = kLpaEmpty;
        sums[s] = 0u;
    }
    lpa_wave_sync();
    bool fail = false;
    rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
        uint32_t l[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool valid = c[u] < a.n && c[u] != row;
            l[u] = valid ? a.label[c[u]] : kLpaEmpty;
            w[u] = valid && a.weight ? a.weight[base + 64u * u + lane] : 1u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (l[u] == kLpaEmpty) continue;
            const uint32_t m = lpa_mix(l[u]);
            if (((m >> 12) & parts_mask) != part) continue;
            uint32_t h = m & mask;
            bool placed = false;
            for (uint32_t i = 0; i < probes; i++) {
                const uint32_t key = atomicCAS(&keys[h], kLpaEmpty, l[u]);
                if (key == kLpaEmpty || key == l[u]) {
                    atomicAdd(&sums[h], w[u]);
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
    long long cs = kLvNoScore;
    uint32_t cl = kLpaEmpty;
    for (uint32_t s = lane; s <= mask; s += 64u) {
        const uint32_t key = keys[s];
        if (key == kLpaEmpty || key == own) continue;
        const long long sc = two_m * (long long)sums[s] - kv * (long long)a.tot[key];
        if (louvain_better(sc, key, cs, cl)) {
            cs = sc;
            cl = key;
        }
    }
    const long long top = (long long)(lpa_wave_max((unsigned long long)cs ^ (1ull << 63)) ^ (1ull << 63));
    const uint32_t first = louvain_wave_min(cs == top ? cl : kLpaEmpty);
    if (first != kLpaEmpty && louvain_better(top, first, best, bl)) {
        best = top;
        bl = first;
    }
    const uint32_t m = lpa_mix(own);
    if (((m >> 12) & parts_mask) == part) {                       // (uniform: every lane looks the same slots up)
        uint32_t h = m & mask;
        for (uint32_t i = 0; i < probes; i++) {
            const uint32_t key = keys[h];
            if (key == own) kin_own = sums[h];
            if (key == own || key == kLpaEmpty) break;
            h = (h + 1u) & mask;
        }
    }
    lpa_wave_sync();                                              // (the next pass clears the table)
    return false;
}

extern __shared__ uint32_t louvain_tables[];                      // per wavefront: table_mask + 1 keys, then as many sums

__global__ __launch_bounds__(256) void louvain_class_kernel(LouvainArgs a, uint32_t cls, uint32_t parity) {
    if (a.ctl[kLvDone] != 0u) return;
    const uint32_t lo = a.offs[cls], hi = a.offs[cls + 1u];
    const long long two_m = (long long)*lv_u64(a.ctl, kLvTwoM);
    const bool first_sweep = a.ctl[kLvSweeps] == 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *keys = louvain_tables + (size_t)wave * 2u * (a.table_mask + 1u), *sums = keys + (a.table_mask + 1u);
    const uint32_t count = hi - lo, nwaves = gridDim.x * 4u;
    // listed vertices per wavefront: 64, fewer when the slice is shorter than the launch (as lpa_class_kernel)
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t nwords = (uint32_t)(((uint64_t)count + per - 1u) / per);
    uint32_t evals = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t item = (uint64_t)wd * per + lane;
        const bool in = lane < per && item < count;
        uint32_t v = 0, beg = 0, end = 0, own = 0, fresh = 0, kvw = 0, tot_own = 0;
        bool moved = false;
        if (in) {
            v = a.list[lo + item];
            beg = a.row_ptr[v] - a.nz_base;
            end = a.row_ptr[v + 1u] - a.nz_base;
            const bool linked = end - beg > 1u || (end - beg == 1u && a.row_idx[beg] != v);
            if (linked) {
                own = a.label[v];
                kvw = a.k[v];
                tot_own = a.tot[own];
                evals += 1u;
            } else {
                end = beg;
            }
        }
        if (beg < end && end - beg <= a.cut) {                    // a thread's row: cut <= kLvThreadMax entries, in registers
            uint32_t c[kLvThreadMax], w[kLvThreadMax], l[kLvThreadMax], t[kLvThreadMax];
#pragma unroll
            for (uint32_t u = 0; u < kLvThreadMax; u++) {
                c[u] = end - beg > u ? a.row_idx[beg + u] : kLpaEmpty;
                w[u] = end - beg > u && a.weight ? a.weight[beg + u] : 1u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kLvThreadMax; u++) {
                const bool valid = c[u] < a.n && c[u] != v;
                l[u] = valid ? a.label[c[u]] : kLpaEmpty;
                w[u] = valid ? w[u] : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kLvThreadMax; u++) t[u] = l[u] != kLpaEmpty ? a.tot[l[u]] : 0u;
            const long long kv = kvw;
            long long best = kLvNoScore;
            uint32_t bl = kLpaEmpty, kin_own = 0;
#pragma unroll
            for (uint32_t i = 0; i < kLvThreadMax; i++) {
                uint32_t kin = 0;
#pragma unroll
                for (uint32_t j = 0; j < kLvThreadMax; j++) kin += l[j] == l[i] ? w[j] : 0u;
                if (l[i] != kLpaEmpty && l[i] != own) {
                    const long long sc = two_m * (long long)kin - kv * (long long)t[i];
                    if (louvain_better(sc, l[i], best, bl)) {
                        best = sc;
                        bl = l[i];
                    }
                }
                kin_own += l[i] == own ? w[i] : 0u;
            }
            const long long cur = two_m * (long long)kin_own - kv * ((long long)tot_own - kv);
            if (bl != kLpaEmpty && best > cur) {
                moved = true;
                fresh = bl;
            }
            beg = end;
        }
        rows_walk_takeover(beg, end, [&](int srcl, uint32_t b, uint32_t e) {
            const uint32_t row = __shfl(v, srcl), mylabel = __shfl(own, srcl);
            const long long kv = (uint32_t)__shfl(kvw, srcl), mytot = (uint32_t)__shfl(tot_own, srcl);
            long long best = kLvNoScore;
            uint32_t bl = kLpaEmpty, kin_own = 0;
            bool stuck = false;
            for (uint32_t parts = 1u;;) {
                best = kLvNoScore;
                bl = kLpaEmpty;
                kin_own = 0u;
                bool overflow = false;
                for (uint32_t part = 0; part < parts && !overflow; part++)
                    overflow = louvain_sum_pass(a, keys, sums, b, e, lane, row, mylabel, two_m, kv, parts - 1u, part, best, bl, kin_own);
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
                if (lane == 0u) ga_store(a.ctl + kLvStuck, 1u);
                return;
            }
            const long long cur = two_m * (long long)kin_own - kv * (mytot - kv);
            if (bl != kLpaEmpty && best > cur && (int)lane == srcl) {      // (every lane holds the same best, bl and cur)
                moved = true;
                fresh = bl;
            }
        });
        const uint32_t pos = wave_append(moved, a.ctl + kLvTail + parity, lane);
        if (moved && pos < a.n) {                                 // (pos < n: every vertex is listed once)
            a.movers[2u * (size_t)pos] = v;
            a.movers[2u * (size_t)pos + 1u] = fresh;
        }
    }
    evals = lpa_wave_sum(evals);
    if (lane == 0u && evals != 0u) ga_add(lv_u64(a.ctl, kLvSweepEvals), (unsigned long long)evals);
}

// behind a class launch: its moves, applied to label and tot
__global__ __launch_bounds__(256) void louvain_apply_kernel(LouvainArgs a, uint32_t parity) {
    if (a.ctl[kLvDone] != 0u) return;
    const uint32_t count = min(a.ctl[kLvTail + parity], a.n);
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
        const uint32_t v = a.movers[2u * i], to = a.movers[2u * i + 1u];
        if (v >= a.n || to >= a.n) continue;                      // (never: the class launch wrote both)
        const uint32_t from = a.label[v], kv = a.k[v];
        a.label[v] = to;
        ga_sub(a.tot + from, kv);
        ga_add(a.tot + to, kv);
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        a.ctl[kLvSweepMoves] += count;
        a.ctl[kLvTail + (parity ^ 1u)] = 0u;                      // the next class launch appends behind this word
    }
}

// behind a sweep's q launch, a launch of its own.  Plain: the words whose stored value depends on the value loaded (sweeps, the
// 64-bit totals of moves and evaluations: the store waits for the load), and the words only read (two_m, stuck) or only
// written (reason, done).  Through the atomic wrappers: every word that is read and then overwritten with a value that does not
// depend on the read -- the sweep's moves and evaluations, In, the sum of squares (louvain_take) and q_last
__global__ void louvain_turn_kernel(uint32_t *ctl, uint32_t max_sweeps, unsigned long long min_gain) {
    if (threadIdx.x != 0u || blockIdx.x != 0u || ctl[kLvDone] != 0u) return;
    const uint32_t moved = louvain_take(ctl + kLvSweepMoves);
    *lv_u64(ctl, kLvMoves) += moved;
    *lv_u64(ctl, kLvEvals) += louvain_take(lv_u64(ctl, kLvSweepEvals));
    const long long before = (long long)ga_load(lv_u64(ctl, kLvQLast)), q = louvain_take_q(ctl, *lv_u64(ctl, kLvTwoM));
    ga_store(lv_u64(ctl, kLvQLast), (unsigned long long)q);
    const uint32_t sweeps = ctl[kLvSweeps] + 1u;
    ctl[kLvSweeps] = sweeps;
    if (ctl[kLvStuck] != 0u) {
        ctl[kLvStuckSeen] = ctl[kLvDone] = 1u;
    } else if (moved == 0u) {
        ctl[kLvReason] = ctl[kLvDone] = 1u;
    } else if (q <= before || (unsigned long long)(q - before) <= min_gain) {
        ctl[kLvReason] = 2u;
        ctl[kLvDone] = 1u;
    } else if (sweeps >= max_sweeps) {
        ctl[kLvDone] = 1u;                                        // (reason 0)
    }
}

// the words of the plan's scratch behind the control record: k, tot, the class list, the histogram (then the scatter's cursors)
// of n words each, n + 1 class offsets, and 2 n words of mover list
constexpr size_t louvain_scratch_bytes(size_t n) { return kRoundsCtlBytes + 4u * (7u * n + 1u); }

static int louvain_move(gl_spmv_plan p, const uint32_t *d_weight, const uint32_t *d_vertex_weight, const uint32_t *d_color, uint32_t *d_label,
                        uint32_t max_sweeps, uint64_t min_gain, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_simple");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    if (h_stats) {
        h_stats[0] = h_stats[4] = 1u;
        h_stats[1] = h_stats[2] = h_stats[3] = h_stats[5] = h_stats[6] = 0u;
    }
    if (n == 0u) return GL_OK;
    if (p->nnz == 0) {                                            // no entries: nobody has a neighbour, the first sweep is empty
        rc = rows_iota(d_label, n);
        if (rc == GL_OK && h_stats) h_stats[3] = 1u;
        return rc;
    }
    rc = plan_scratch(p->d_louvain_scratch, louvain_scratch_bytes(n),
                      who, "control record, vertex weights, community totals, class list, histogram, offsets and mover list");
    if (rc != GL_OK) return rc;
    uint32_t *ctl = reinterpret_cast<uint32_t *>(p->d_louvain_scratch);
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    static_assert(kLvRecordWords * 4u <= 64u && (kLvReadEnd - kLpaTop) * 4u <= 64u, "either read-back fits the page-locked staging words");
    const auto word = [&](uint32_t k) { return w[k - kLpaTop]; }; // a word of the second line, as the first read-back left it
    const auto wide = [&](uint32_t k) { return (uint64_t)w[k] | ((uint64_t)w[k + 1u] << 32); };
    const unsigned vertex_grid = rows_stream_grid(n);
    LouvainArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.weight = d_weight;
    a.ctl = ctl;
    a.label = d_label;
    a.k = ctl + kRoundsCtlBytes / 4u;
    a.tot = a.k + n;
    uint32_t *list = a.tot + n, *hist = list + n, *offs = hist + n;
    a.movers = offs + n + 1u;
    a.list = list;
    a.offs = offs;
    a.n = n;
    a.nz_base = p->csr_nz_base;
    GL_HIP(hipMemsetAsync(ctl, 0, kRoundsCtlBytes, s));
    GL_HIP(hipMemsetAsync(hist, 0, 4u * (size_t)n, s));
    louvain_rows_kernel<true><<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, d_weight, d_vertex_weight, n, a.nz_base, d_label, a.k, a.tot, ctl);
    lpa_check_kernel<<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, d_color, n, a.nz_base, hist, ctl);
    lpa_scan_kernel<<<1, 1024, 0, s>>>(hist, offs, ctl, n);
    lpa_scatter_kernel<<<vertex_grid, 256, 0, s>>>(d_color, n, hist, list);
    louvain_rows_kernel<false><<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, d_weight, nullptr, n, a.nz_base, d_label, a.k, a.tot, ctl);
    louvain_begin_kernel<<<1, 64, 0, s>>>(ctl);
    uint64_t launches = 6;
    GL_LAUNCH_CHECK();
    GL_HIP(hipMemcpyAsync(w, ctl + kLpaTop, (kLvReadEnd - kLpaTop) * 4u, hipMemcpyDeviceToHost, s));
    GL_HIP(hipStreamSynchronize(s));
    if (word(kLpaBadColor) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: %u words of d_color hold a colour >= n = %u (d_label is then written, and not a result)", who,
                         word(kLpaBadColor), n);
    if (word(kLpaImproper) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: d_color is not a proper colouring: %u entries (v, u) have colour[v] == colour[u], so two "
                         "vertices of one class launch would decide from each other's labels (gl_color gives a proper one; d_label is "
                         "then written, and not a result)", who, word(kLpaImproper));
    if (word(kLvBadWeight) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: %u words of d_weight are zero: an entry of the pattern is an edge, and its weight is at "
                         "least 1 (d_label is then written, and not a result)", who, word(kLvBadWeight));
    if (word(kLvBadK) != 0u)
        return set_error(GL_ERR_INVALID_ARG, "%s: %u words of d_vertex_weight are below the sum of their vertex's entry weights: k[v] is "
                         "that sum plus the vertex's internal weight (d_label is then written, and not a result)", who, word(kLvBadK));
    const uint64_t two_m = (uint64_t)word(kLvSumK) | ((uint64_t)word(kLvSumK + 1u) << 32);
    if (two_m >= (1ull << 31))
        return set_error(GL_ERR_UNSUPPORTED, "%s: the vertex weights sum to two_m = %llu >= 2^31: the scores are 64-bit integers, and their "
                         "products stay below 2^62 only under that bound (d_label is then written, and not a result)", who,
                         (unsigned long long)two_m);
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 25): louvain_cut = entries of a row that a thread sums in
    // registers (0 .. 8; longer rows go to the wavefront), louvain_grid = workgroups per compute unit of a class launch,
    // louvain_batch = sweeps enqueued between two read-backs of the control record, louvain_table = slots of a wavefront's LDS table
    // (a power of two, 8 .. 2048)
    const uint32_t classes = word(kLpaTop) + 1u;
    const RowsWalkShape shape = rows_walk_shape(n, 0, 0, debug_knob("louvain_grid", 8));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("louvain_batch", 4), 64));
    uint32_t table = 8;
    while (table < 2048u && (long)table < debug_knob("louvain_table", 2048)) table <<= 1;
    a.cut = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("louvain_cut", kLvThreadMax), kLvThreadMax));
    a.table_mask = table - 1u;
    const size_t lds = 4u * 2u * (size_t)table * sizeof(uint32_t);      // four wavefronts' keys and sums: 64 KiB at most
    uint32_t parity = 0;                                          // of the class launches enqueued so far: which tail they append to
    rc = rounds_run(
        batch, (uint64_t)max_sweeps + batch, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                for (uint32_t c = 0; c < classes; c++, parity ^= 1u) {
                    louvain_class_kernel<<<shape.grid, 256, lds, s>>>(a, c, parity);
                    louvain_apply_kernel<<<shape.grid, 256, 0, s>>>(a, parity);
                }
                louvain_rows_kernel<false><<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, d_weight, nullptr, n, a.nz_base, d_label, a.k, a.tot, ctl);
                louvain_turn_kernel<<<1, 64, 0, s>>>(ctl, max_sweeps, (unsigned long long)min_gain);
            }
            return (uint64_t)batch * (2ull * classes + 2u);
        },
        [&] { return hipMemcpyAsync(w, ctl, kLvRecordWords * 4u, hipMemcpyDeviceToHost, s); },
        [&] { return w[kLvStuckSeen] != 0u ? kRoundsStuck : w[kLvDone] != 0u ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t sweeps) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu sweeps of %u allowed on %u vertices (%u sweeps counted%s)", who,
                             (unsigned long long)sweeps, max_sweeps, n, w[kLvSweeps],
                             w[kLvStuckSeen] ? "; a row's labels did not fit the table in 2^20 partitions" : "");
        });
    if (rc != GL_OK) return rc;
    if (h_stats) {
        h_stats[0] = w[kLvSweeps];
        h_stats[1] = wide(kLvMoves);
        h_stats[2] = wide(kLvEvals);
        h_stats[3] = launches;
        h_stats[4] = w[kLvReason];
        h_stats[5] = wide(kLvQFirst);
        h_stats[6] = wide(kLvQLast);
    }
    return GL_OK;
}

}  // namespace gl

int gl_louvain_move(gl_spmv_plan plan, const uint32_t *d_weight, const uint32_t *d_vertex_weight, const uint32_t *d_color, uint32_t *d_label,
                    uint32_t max_sweeps, uint64_t min_gain, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_color != nullptr && d_label != nullptr);
    GL_ARG(max_sweeps != 0u);
    GL_ARG(d_color != d_label);
    return gl::louvain_move(plan, d_weight, d_vertex_weight, d_color, d_label, max_sweeps, min_gain, h_stats, "gl_louvain_move");
}
