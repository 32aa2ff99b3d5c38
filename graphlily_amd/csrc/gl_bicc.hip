// Biconnected components (gl_bicc): Tarjan and Vishkin's algorithm over a DETERMINISTIC BFS forest of the plain CSR copy that a
// GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base) -- a square whole-matrix plan whose rows
// are strictly ascending sets of columns below num_cols and whose pattern is symmetric, over n = num_rows vertices.  Entry j is
// word j of the row copy; an edge is the pair of entries (v, u) and (u, v); an entry (v, v) belongs to no block.
// Every array below is a pure function of the graph (include/graphlily_hip_bicc.h states the public contract):
//   1 roots     gl_cc's begin / hook / doubling: r is a root iff label[r] == r (isolated vertices included)
//   2 level     multi-source BFS from all roots: a queue seeded with the roots grows while it is consumed, one gated launch per
//               level; a vertex is claimed by a compare-and-swap on its level word; the turn records level_start[d], so the
//               finished queue is the vertices grouped by level (the ORDER inside a level is the only thing here that is not
//               unique, and nothing depends on it)
//   3 parent    parent[v] = the smallest neighbour one level up (rows ascend: the first match ends the row); parent[root] = root
//   4 nd        subtree sizes, level by level from the deepest: nd[parent[v]] += nd[v]
//   5 pre       preorder, local to each tree, level by level from the top: pre[root] = 0; vertex v walks its own row and gives its
//               children (parent[u] == v), in ascending order, pre[v] + 1 + the nd of the earlier children
//   6 low/high  low[v] = min of pre[v] and pre[u] over the non-tree neighbours u (neither end is the other's parent), then pushed
//               to the parents level by level from the deepest; high the same with max
//   7 blocks    a tree edge is named by its child; union-find over n words (gl_unionfind.h): for a tree edge v -> w, v no root,
//               unite (v, w) iff low[w] < pre[v] || high[w] >= pre[v] + nd[v]; for a non-tree entry (v, w) with pre[v] + nd[v]
//               <= pre[w] unite (v, w); then pointer doubling
//   8 labels    the child that names an entry's block is the child end of a tree edge and the end with the larger pre of a
//               non-tree edge; first[root] = the smallest entry of the class (atomic min), block[j] = first[root]
//   9 results   bridges: a tree edge to c with low[c] >= pre[c] && high[c] < pre[c] + nd[c]; every block has one top vertex, the
//               parent of its shallowest child (a 64-bit atomic min of level << 32 | child per class): vertex_blocks[v] = (v is no
//               root) + the blocks whose top is v; edge_component = begin / hook / doubling again, the hook skipping bridges
// MEMORY RULE and GATING: gl_rounds.h.  What is atomic-only in which launch:
//   * level step   level[] (a relaxed load, a compare-and-swap) and the queue's tail; the queue is read below the slice's end and
//                  written behind it;
//   * nd push      nd[] of the parents by atomic add (the words of the slice's own level are read plainly: nobody writes them);
//   * low / high   low[] and high[] of the parents by atomic min / max, likewise;
//   * unite        uf[]: gl_cc.hip's discipline;   * first: first[] by atomic min;   * tops: top[] by 64-bit atomic min, cnt[] by
//                  atomic add;   * every counter of the control record by one atomic add per wavefront.
// Everything else is read behind the launch boundary that wrote it.  No spin-waits, no tickets: every wait is a launch boundary.
// STEP CAP: a level step that does not end the search finds a level that is not empty, and there are at most n levels: n steps.
// The sweeps over the levels (4, 5, the push of 6) are enqueued blindly once `depth` is known -- depth launches each -- and read
// their slice [level_start[d], level_start[d + 1]) on the device.
// SCRATCH, per plan: 256 + 4 (16 n + 2) bytes -- the control record, top (8 n), the six tree arrays, the queue, the roots' labels,
// uf and its labels, first, the bridge flags, cnt, and level_start (n + 2).
#include "gl_unionfind.h"
#include "graphlily_hip_bicc.h"

namespace gl {

// the control record (words): the first line is the turn's, the second is added to by the launches
enum : uint32_t { kBiLo = 0, kBiHi = 1, kBiDepth = 2, kBiDone = 3, kBiTrees = 4, kBiRecordWords = 5, kBiTail = 32, kBiBlocks = 33, kBiArt = 34,
                  kBiBridges = 35, kBiCountWords = 4 };
constexpr uint32_t kBiNone = 0xffffffffu;

struct BiccArgs {
    const uint32_t *row_ptr, *row_idx;
    uint32_t *ctl, *level, *parent, *pre, *nd, *low, *high, *queue, *lstart, *root, *uf, *ufl, *first, *flag, *cnt, *block;
    unsigned long long *top;
    uint32_t n, nz_base, cut_steps;
};

// one atomic add per wavefront: `mine` = this lane's count (every lane of the wavefront calls it)
__device__ __forceinline__ void bicc_count(uint32_t *word, uint32_t mine, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) mine += (uint32_t)__shfl_xor(mine, d);
    if (lane == 0u && mine != 0u) ga_add(word, mine);
}

// The rows of list[lo .. hi) (list == nullptr: of the vertices lo .. hi) dealt to the wavefronts of the launch as gl_scc deals
// its lists: 64 per wavefront, fewer when the slice is shorter than the launch; a wavefront with ONE row gives it to all its lanes
// at once.  f(v, in, beg, end, steps, lane) runs in every lane, `in` says whether the lane has a row.
template <typename F>
__device__ __forceinline__ void bicc_rows(const BiccArgs &a, const uint32_t *list, uint32_t lo, uint32_t hi, F &&f) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = hi - lo, nwaves = gridDim.x * 4u;
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t words = (uint32_t)(((uint64_t)count + per - 1u) / per);
    const uint32_t steps = per == 1u ? 0u : a.cut_steps;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < words; wd += nwaves) {
        const uint64_t i = (uint64_t)wd * per + lane;
        const bool in = lane < per && i < count;
        uint32_t v = 0, beg = 0, end = 0;
        if (in) {
            v = list ? list[lo + (uint32_t)i] : lo + (uint32_t)i;
            beg = a.row_ptr[v] - a.nz_base;
            end = a.row_ptr[v + 1u] - a.nz_base;
        }
        f(v, in, beg, end, steps, lane);
    }
}

// Every vertex: the state of the later phases, and the roots into the queue (plain stores: nobody reads these words here).
__global__ __launch_bounds__(256) void bicc_seed_kernel(BiccArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)a.n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        bool is_root = false;
        if (v64 < a.n) {
            is_root = a.root[v] == v;
            a.level[v] = is_root ? 0u : kBiNone;
            a.pre[v] = 0u;
            a.nd[v] = 1u;
            a.uf[v] = v;
            a.first[v] = kBiNone;
            a.top[v] = ~0ull;
            a.flag[v] = 0u;
            a.cnt[v] = 0u;
        }
        const uint32_t at = wave_append(is_root, a.ctl + kBiTail, lane);
        if (is_root && at < a.n) a.queue[at] = v;
    }
}

// Behind the seed and behind every level step (one thread, plain loads and stores: a launch of its own): the slice that the step
// appended becomes the next level; none, or a queue that holds every vertex, ends the search.
__global__ void bicc_turn_kernel(uint32_t *ctl, uint32_t *lstart, uint32_t n, uint32_t seed) {
    if (blockIdx.x != 0u || threadIdx.x != 0u || ctl[kBiDone] != 0u) return;
    const uint32_t lo = seed ? 0u : ctl[kBiHi], hi = min(ctl[kBiTail], n);
    uint32_t d = ctl[kBiDepth];
    if (seed) {
        lstart[0] = 0u;
        ctl[kBiLo] = 0u;
        ctl[kBiHi] = hi;
        ctl[kBiTrees] = hi;
    } else if (hi > lo) {
        d += 1u;
        lstart[d] = lo;
        ctl[kBiDepth] = d;
        ctl[kBiLo] = lo;
        ctl[kBiHi] = hi;
    }
    if (hi == lo || hi == n) {
        lstart[d + 1u] = hi;
        ctl[kBiDone] = 1u;
    }
}

// one level: the vertices of the slice claim their unreached neighbours for the next level and append them to the queue
__global__ __launch_bounds__(256) void bicc_level_kernel(BiccArgs a) {
    if (a.ctl[kBiDone] != 0u) return;
    const uint32_t lo = a.ctl[kBiLo], hi = min(a.ctl[kBiHi], a.n), next = a.ctl[kBiDepth] + 1u;
    if (lo >= hi) return;
    bicc_rows(a, a.queue, lo, hi, [&](uint32_t, bool, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        // (the append aggregates over the lanes that take the step: its ballot, its leader and its shuffle are theirs)
        auto claim = [&](const uint32_t(&c)[4]) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                bool won = false;
                if (c[u] < a.n && ga_load(a.level + c[u]) == kBiNone) {
                    uint32_t seen = kBiNone;
                    won = ga_cas(a.level + c[u], seen, next);
                }
                const uint32_t at = wave_append(won, a.ctl + kBiTail, lane);
                if (won && at < a.n) a.queue[at] = c[u];              // (at < n: a vertex is claimed once)
            }
        };
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
            claim(c);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int, uint32_t b, uint32_t e) {
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                claim(c);
                return false;
            });
        });
    });
}

// parent[v] = the smallest neighbour one level up: gl_bfs_parents' rule on ascending rows, the first match ends the row
__global__ __launch_bounds__(256) void bicc_parent_kernel(BiccArgs a) {
    bicc_rows(a, nullptr, 0u, a.n, [&](uint32_t v, bool in, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        const uint32_t lv = in ? a.level[v] : 0u;
        const uint32_t want = lv - 1u;
        if (lv == 0u || lv == kBiNone) beg = end;
        uint32_t best = kBiNone;
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
            uint32_t l[4];
#pragma unroll
            for (int u = 0; u < 4; u++) l[u] = c[u] < a.n ? a.level[c[u]] : kBiNone;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.n && l[u] == want) best = min(best, c[u]);
            return best != kBiNone;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t w = __shfl(want, src);
            uint32_t m = kBiNone;
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                uint32_t l[4];
#pragma unroll
                for (int u = 0; u < 4; u++) l[u] = c[u] < a.n ? a.level[c[u]] : kBiNone;
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n && l[u] == w) m = min(m, c[u]);
                return __any(m != kBiNone) != 0;
            });
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) m = min(m, (uint32_t)__shfl_xor(m, d));
            if ((int)lane == src) best = m;
        });
        if (in) a.parent[v] = lv == 0u ? v : best;
    });
}

// the pushes to the parents, over the slice of level d >= 1 (a thread per vertex): WHAT = 0 adds nd, 1 takes low / high
template <int WHAT>
__global__ __launch_bounds__(256) void bicc_push_kernel(BiccArgs a, uint32_t d) {
    const uint32_t lo = a.lstart[d], hi = min(a.lstart[d + 1u], a.n);
    for (uint64_t i = (uint64_t)lo + blockIdx.x * 256u + threadIdx.x; i < hi; i += gridDim.x * 256u) {
        const uint32_t v = a.queue[i], p = a.parent[v];
        if (p >= a.n || p == v) continue;
        if (WHAT == 0) {
            ga_add(a.nd + p, a.nd[v]);
        } else {
            ga_min(a.low + p, a.low[v]);
            ga_max(a.high + p, a.high[v]);
        }
    }
}

// exclusive prefix sum over the 64 lanes; `total` = the sum of all of them
__device__ __forceinline__ uint32_t bicc_wave_scan(uint32_t x, uint32_t lane, uint32_t &total) {
    uint32_t incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += up;
    }
    total = (uint32_t)__shfl(incl, 63);
    return incl - x;
}

// preorder numbers of the children of the slice of level d: a running sum per thread, and across the wavefront's 256-entry steps
// an exclusive prefix sum in ENTRY order -- lane l holds the entries base + 64 u + l, so the four u are scanned one after the other
__global__ __launch_bounds__(256) void bicc_pre_kernel(BiccArgs a, uint32_t d) {
    const uint32_t lo = a.lstart[d], hi = min(a.lstart[d + 1u], a.n);
    if (lo >= hi) return;
    bicc_rows(a, a.queue, lo, hi, [&](uint32_t v, bool in, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        uint32_t run = in ? a.pre[v] + 1u : 0u;
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
            uint32_t p[4];
#pragma unroll
            for (int u = 0; u < 4; u++) p[u] = c[u] < a.n ? a.parent[c[u]] : kBiNone;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.n && c[u] != v && p[u] == v) {
                    a.pre[c[u]] = run;
                    run += a.nd[c[u]];
                }
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vr = __shfl(v, src);
            uint32_t carry = __shfl(run, src);
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                uint32_t p[4], x[4];
#pragma unroll
                for (int u = 0; u < 4; u++) p[u] = c[u] < a.n ? a.parent[c[u]] : kBiNone;
#pragma unroll
                for (int u = 0; u < 4; u++) x[u] = c[u] < a.n && c[u] != vr && p[u] == vr ? a.nd[c[u]] : 0u;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    uint32_t total;
                    const uint32_t before = bicc_wave_scan(x[u], lane, total);
                    if (x[u] != 0u) a.pre[c[u]] = carry + before;     // (nd >= 1: x != 0 says child)
                    carry += total;
                }
                return false;
            });
        });
    });
}

// low[v] / high[v] = min / max of pre[v] and pre[u] over the non-tree neighbours u
__global__ __launch_bounds__(256) void bicc_lowhigh_kernel(BiccArgs a) {
    bicc_rows(a, nullptr, 0u, a.n, [&](uint32_t v, bool in, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        const uint32_t pv = in ? a.pre[v] : 0u, par = in ? a.parent[v] : kBiNone;
        uint32_t lw = pv, hg = pv;
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
            uint32_t p[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                p[u] = c[u] < a.n ? a.parent[c[u]] : kBiNone;
                q[u] = c[u] < a.n ? a.pre[c[u]] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.n && c[u] != v && p[u] != v && par != c[u]) {
                    lw = min(lw, q[u]);
                    hg = max(hg, q[u]);
                }
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vr = __shfl(v, src), pr = __shfl(par, src);
            uint32_t l2 = kBiNone, h2 = 0u;
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                uint32_t p[4], q[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    p[u] = c[u] < a.n ? a.parent[c[u]] : kBiNone;
                    q[u] = c[u] < a.n ? a.pre[c[u]] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n && c[u] != vr && p[u] != vr && pr != c[u]) {
                        l2 = min(l2, q[u]);
                        h2 = max(h2, q[u]);
                    }
                return false;
            });
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                l2 = min(l2, (uint32_t)__shfl_xor(l2, d));
                h2 = max(h2, (uint32_t)__shfl_xor(h2, d));
            }
            if ((int)lane == src) {
                lw = min(lw, l2);
                hg = max(hg, h2);
            }
        });
        if (in) {
            a.low[v] = lw;
            a.high[v] = hg;
        }
    });
}

// the two rules of phase 7 over the entries of every row; uf[] is atomic-only (gl_cc.hip's discipline)
__global__ __launch_bounds__(256) void bicc_unite_kernel(BiccArgs a) {
    bicc_rows(a, nullptr, 0u, a.n, [&](uint32_t v, bool in, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        const uint32_t pv = in ? a.pre[v] : 0u, par = in ? a.parent[v] : kBiNone;
        const uint32_t behind = in ? pv + a.nd[v] : 0u;             // the first preorder number behind v's subtree
        // is the edge named by w in the class of the edge named by v?  (self: the row's vertex, its preorder number, ...)
        auto joins = [&](uint32_t w, uint32_t self, uint32_t self_par, uint32_t self_pre, uint32_t self_behind) {
            if (w >= a.n || w == self) return false;
            if (a.parent[w] == self) return self_par != self && (a.low[w] < self_pre || a.high[w] >= self_behind);
            return self_par != w && self_behind <= a.pre[w];
        };
        uint32_t anc = v;                                           // an ancestor-or-self of v in uf: only ever descends
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
            bool j[4];
#pragma unroll
            for (int u = 0; u < 4; u++) j[u] = joins(c[u], v, par, pv, behind);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (j[u]) anc = cc_unite(a.uf, anc, c[u]);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vr = __shfl(v, src), pr = __shfl(par, src), pvr = __shfl(pv, src), br = __shfl(behind, src);
            uint32_t av = __shfl(anc, src);
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                bool j[4];
#pragma unroll
                for (int u = 0; u < 4; u++) j[u] = joins(c[u], vr, pr, pvr, br);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (j[u]) av = cc_unite(a.uf, av, c[u]);
                return false;
            });
        });
    });
}

// phase 8 over the entries of every row: WRITE = false takes the minimum entry number per class, true writes the labels
template <bool WRITE>
__global__ __launch_bounds__(256) void bicc_entries_kernel(BiccArgs a) {
    bicc_rows(a, nullptr, 0u, a.n, [&](uint32_t v, bool in, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        const uint32_t pv = in ? a.pre[v] : 0u, par = in ? a.parent[v] : kBiNone;
        // A lane meets its entries in ascending order, so of a run of entries of one class only the first can lower the minimum;
        // and one whose number the word already undercuts needs no atomic either.  Without the two tests every entry of a giant
        // block is an atomic on ONE word: 280 of the 297 ms of the call on the orkut stand-in (EXPERIMENTS.md Round 27).
        uint32_t last = kBiNone;
        auto entry = [&](uint32_t w, uint32_t j, uint32_t self, uint32_t self_par, uint32_t self_pre) {
            if (w >= a.n) return;                                   // (padding; the contract admits no zero-valued entry)
            if (w == self) {
                if (WRITE) a.block[j] = kBiNone;
                return;
            }
            const uint32_t child = a.parent[w] == self ? w : self_par == w ? self : a.pre[w] > self_pre ? w : self;
            const uint32_t r = a.ufl[child];
            if (WRITE) {
                a.block[j] = a.first[r];
            } else if (r != last) {
                last = r;
                if (j < ga_load(a.first + r)) ga_min(a.first + r, j);
            }
        };
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t at) {
#pragma unroll
            for (int u = 0; u < 4; u++) entry(c[u], at + (uint32_t)u, v, par, pv);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vr = __shfl(v, src), pr = __shfl(par, src), pvr = __shfl(pv, src);
            last = kBiNone;                                         // (another row: its entries may lie below the lane's last one)
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
#pragma unroll
                for (int u = 0; u < 4; u++) entry(c[u], (uint32_t)(base + 64u * (uint32_t)u + lane), vr, pr, pvr);
                return false;
            });
        });
    });
}

// phase 9, a thread per vertex, three launches: STEP 0 flags and counts the bridges and finds every class's shallowest child;
// 1 counts the blocks and gives each to its top vertex; 2 writes vertex_blocks and counts the articulation points
template <int STEP>
__global__ __launch_bounds__(256) void bicc_vertex_kernel(BiccArgs a, uint32_t *vertex_blocks) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    const uint64_t nround = ((uint64_t)a.n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        if (v64 >= a.n) continue;
        const bool child = a.parent[v] != v;                        // v names a tree edge
        if (STEP == 0 && child) {
            const uint32_t pv = a.pre[v];
            if (a.low[v] >= pv && a.high[v] < pv + a.nd[v]) {
                a.flag[v] = 1u;
                mine += 1u;
            }
            const unsigned long long key = ((unsigned long long)a.level[v] << 32) | v;
            unsigned long long *word = a.top + a.ufl[v];
            if (key < ga_load(word)) ga_min(word, key);              // (the test: a giant block is ONE word for all its vertices)
        }
        if (STEP == 1 && child && a.ufl[v] == v) {
            const uint32_t shallowest = (uint32_t)a.top[v];
            if (shallowest < a.n) ga_add(a.cnt + a.parent[shallowest], 1u);
            mine += 1u;
        }
        if (STEP == 2) {
            const uint32_t blocks = (child ? 1u : 0u) + a.cnt[v];
            if (vertex_blocks) vertex_blocks[v] = blocks;
            mine += blocks >= 2u ? 1u : 0u;
        }
    }
    bicc_count(a.ctl + (STEP == 0 ? kBiBridges : STEP == 1 ? kBiBlocks : kBiArt), mine, lane);
}

// gl_cc's hook without the bridges: the components of what is left are the 2-edge-connected components
__global__ __launch_bounds__(256) void bicc_hook_kernel(BiccArgs a) {
    bicc_rows(a, nullptr, 0u, a.n, [&](uint32_t v, bool in, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane) {
        const uint32_t par = in ? a.parent[v] : kBiNone, fv = in ? a.flag[v] : 0u;
        auto keeps = [&](uint32_t w, uint32_t self, uint32_t self_par, uint32_t self_flag) {
            if (w >= a.n || w == self) return false;
            return !(a.parent[w] == self ? a.flag[w] != 0u : self_par == w && self_flag != 0u);
        };
        uint32_t anc = v;
        rows_walk_thread(a.row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
            bool k[4];
#pragma unroll
            for (int u = 0; u < 4; u++) k[u] = keeps(c[u], v, par, fv);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (k[u]) anc = cc_unite(a.uf, anc, c[u]);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vr = __shfl(v, src), pr = __shfl(par, src), fr = __shfl(fv, src);
            uint32_t av = __shfl(anc, src);
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                bool k[4];
#pragma unroll
                for (int u = 0; u < 4; u++) k[u] = keeps(c[u], vr, pr, fr);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (k[u]) av = cc_unite(a.uf, av, c[u]);
                return false;
            });
        });
    });
}

// a graph without entries: every vertex is a tree of its own
__global__ __launch_bounds__(256) void bicc_trivial_kernel(uint32_t *__restrict__ vertex_blocks, uint32_t *__restrict__ tree, uint32_t n) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        if (vertex_blocks) vertex_blocks[v] = 0u;
        if (tree) {
            tree[v] = 0u;                                           // level
            tree[(size_t)n + v] = (uint32_t)v;                      // parent
            tree[2u * (size_t)n + v] = 0u;                          // pre
            tree[3u * (size_t)n + v] = 1u;                          // nd
            tree[4u * (size_t)n + v] = 0u;                          // low
            tree[5u * (size_t)n + v] = 0u;                          // high
        }
    }
}

// the bytes of the plan's scratch: the control record, top (64 bits a vertex), fifteen arrays of n words, level_start (n + 2)
constexpr size_t bicc_scratch_bytes(size_t n) { return kRoundsCtlBytes + 4u * (16u * n + 2u); }

static bool bicc_overlap(const uint32_t *x, size_t nx, const uint32_t *y, size_t ny) {
    return x && y && x < y + std::max<size_t>(ny, 1) && y < x + std::max<size_t>(nx, 1);
}

static int bicc(gl_spmv_plan p, uint32_t *d_block, uint32_t *d_vb, uint32_t *d_ec, uint32_t *d_tree, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_simple");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    const uint64_t nnz = p->nnz;
    if (h_stats) std::fill(h_stats, h_stats + 6, 0ull);
    if (n == 0u) return GL_OK;
    const uint32_t *outs[4] = {d_block, d_vb, d_ec, d_tree};
    const size_t lens[4] = {(size_t)nnz, n, n, 6u * (size_t)n};
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (bicc_overlap(outs[i], lens[i], outs[j], lens[j]))
                return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: the outputs overlap", who);
    const unsigned stream_grid = rows_stream_grid(n);
    if (nnz == 0) {                                               // no entries: n trees, no block
        bicc_trivial_kernel<<<stream_grid, 256, 0, s>>>(d_vb, d_tree, n);
        GL_LAUNCH_CHECK();
        uint64_t launches = 1;
        if (d_ec) {
            if ((rc = rows_iota(d_ec, n)) != GL_OK) return rc;
            launches++;
        }
        GL_HIP(hipStreamSynchronize(s));
        if (h_stats) {
            h_stats[4] = launches;
            h_stats[5] = n;
        }
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 27): bicc_cut = entries a thread reads before the wavefront
    // takes the row over, bicc_grid = workgroups per compute unit of a walk, bicc_batch = (level step, turn) pairs enqueued between
    // two read-backs of the control record.  bicc_stop = 1 / 2 / 3 / 4 is a MEASUREMENT hook (benchmarks/bench_bicc.py times the phases with
    // it): the call ends behind the levels, the forest (phases 3 - 6), the union-find (7) or the labels (8), waits, and leaves the outputs unfinished
    const long stop = debug_knob("bicc_stop", 0);
    auto stopped = [&](uint64_t done) {
        if (h_stats) h_stats[4] = done;
        return hipStreamSynchronize(s);
    };
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("bicc_cut", 32), 1l << 30, debug_knob("bicc_grid", 8));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("bicc_batch", 32), 4096));
    rc = plan_scratch(p->d_bicc_scratch, bicc_scratch_bytes(n), who, "control record, forest, queue, union-find and block tops");
    if (rc != GL_OK) return rc;
    BiccArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.nz_base = p->csr_nz_base;
    a.n = n;
    a.cut_steps = shape.cut_steps;
    a.ctl = reinterpret_cast<uint32_t *>(p->d_bicc_scratch);
    a.top = reinterpret_cast<unsigned long long *>(p->d_bicc_scratch + kRoundsCtlBytes);
    a.level = reinterpret_cast<uint32_t *>(a.top + n);
    a.parent = a.level + n;
    a.pre = a.parent + n;
    a.nd = a.pre + n;
    a.low = a.nd + n;
    a.high = a.low + n;
    a.queue = a.high + n;
    a.root = a.queue + n;
    a.uf = a.root + n;
    a.ufl = a.uf + n;
    a.first = a.ufl + n;
    a.flag = a.first + n;
    a.cnt = a.flag + n;
    a.lstart = a.cnt + n;
    a.block = d_block;
    const unsigned walk_grid = shape.grid;
    uint64_t launches = 0;
    // 1: the roots
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes, s));
    if ((rc = cc_begin(a.uf, n)) != GL_OK || (rc = cc_hook(p, a.uf)) != GL_OK || (rc = cc_double(a.uf, n, a.root, who)) != GL_OK) return rc;
    // 2: the levels
    bicc_seed_kernel<<<stream_grid, 256, 0, s>>>(a);
    bicc_turn_kernel<<<1, 64, 0, s>>>(a.ctl, a.lstart, n, 1u);
    GL_LAUNCH_CHECK();
    launches += 4;                                                // (the doubling rounds are not counted: most return at once)
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    static_assert((kBiRecordWords + kBiCountWords) * 4u <= 64u, "the record and the counters fit the page-locked staging words");
    for (uint32_t i = 0; i < kBiRecordWords + kBiCountWords; i++) w[i] = 0u;
    auto copy_record = [&] {
        const hipError_t e = hipMemcpyAsync(w, a.ctl, kBiRecordWords * 4u, hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipMemcpyAsync(w + kBiRecordWords, a.ctl + kBiTail, kBiCountWords * 4u, hipMemcpyDeviceToHost, s);
    };
    rc = rounds_run(
        batch, n, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                bicc_level_kernel<<<walk_grid, 256, 0, s>>>(a);
                bicc_turn_kernel<<<1, 64, 0, s>>>(a.ctl, a.lstart, n, 0u);
            }
            return 2ull * batch;
        },
        copy_record, [&] { return w[kBiDone] != 0u ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: the search is not done after %llu steps on %u vertices (level %u, slice [%u, %u))",
                             who, (unsigned long long)steps, n, w[kBiDepth], w[kBiLo], w[kBiHi]);
        });
    if (rc != GL_OK) return rc;
    const uint32_t depth = w[kBiDepth], trees = w[kBiTrees];
    if (w[kBiRecordWords] != n || depth >= n)
        return set_error(GL_ERR_HIP, "%s: internal error: the search queued %u of %u vertices on %u levels", who, w[kBiRecordWords], n, depth);
    if (stop == 1) {
        GL_HIP(stopped(launches));
        return GL_OK;
    }
    // 3 - 6: the forest
    bicc_parent_kernel<<<walk_grid, 256, 0, s>>>(a);
    for (uint32_t d = depth; d >= 1u; d--) bicc_push_kernel<0><<<stream_grid, 256, 0, s>>>(a, d);
    for (uint32_t d = 0; d < depth; d++) bicc_pre_kernel<<<walk_grid, 256, 0, s>>>(a, d);
    bicc_lowhigh_kernel<<<walk_grid, 256, 0, s>>>(a);
    for (uint32_t d = depth; d >= 1u; d--) bicc_push_kernel<1><<<stream_grid, 256, 0, s>>>(a, d);
    GL_LAUNCH_CHECK();
    if (stop == 2) {
        GL_HIP(stopped(launches + 3ull * depth + 2ull));
        return GL_OK;
    }
    // 7, 8: the blocks
    bicc_unite_kernel<<<walk_grid, 256, 0, s>>>(a);
    GL_LAUNCH_CHECK();
    if ((rc = cc_double(a.uf, n, a.ufl, who)) != GL_OK) return rc;
    if (stop == 3) {
        GL_HIP(stopped(launches + 3ull * depth + 3ull));
        return GL_OK;
    }
    bicc_entries_kernel<false><<<walk_grid, 256, 0, s>>>(a);
    bicc_entries_kernel<true><<<walk_grid, 256, 0, s>>>(a);
    if (stop == 4) {
        GL_HIP(stopped(launches + 3ull * depth + 5ull));
        return GL_OK;
    }
    // 9: bridges, tops, vertex_blocks, the 2-edge-connected components
    bicc_vertex_kernel<0><<<stream_grid, 256, 0, s>>>(a, nullptr);
    bicc_vertex_kernel<1><<<stream_grid, 256, 0, s>>>(a, nullptr);
    bicc_vertex_kernel<2><<<stream_grid, 256, 0, s>>>(a, d_vb);
    GL_LAUNCH_CHECK();
    launches += 3ull * depth + 8ull;
    if (d_ec) {
        if ((rc = cc_begin(a.uf, n)) != GL_OK) return rc;
        bicc_hook_kernel<<<walk_grid, 256, 0, s>>>(a);
        GL_LAUNCH_CHECK();
        if ((rc = cc_double(a.uf, n, d_ec, who)) != GL_OK) return rc;
        launches += 2;
    }
    if (d_tree) GL_HIP(hipMemcpyAsync(d_tree, a.level, 24u * (size_t)n, hipMemcpyDeviceToDevice, s));
    GL_HIP(copy_record());
    GL_HIP(hipStreamSynchronize(s));
    if (h_stats) {
        h_stats[0] = w[kBiRecordWords + kBiBlocks - kBiTail];
        h_stats[1] = w[kBiRecordWords + kBiArt - kBiTail];
        h_stats[2] = w[kBiRecordWords + kBiBridges - kBiTail];
        h_stats[3] = depth;
        h_stats[4] = launches;
        h_stats[5] = trees;
    }
    return GL_OK;
}

}  // namespace gl

int gl_bicc(gl_spmv_plan plan, uint32_t *d_block, uint32_t *d_vertex_blocks, uint32_t *d_edge_component, uint32_t *d_tree,
            uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_block != nullptr);
    return gl::bicc(plan, d_block, d_vertex_blocks, d_edge_component, d_tree, h_stats, "gl_bicc");
}
