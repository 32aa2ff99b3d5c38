// graphlily/io/data_formatter.h -- the two host formatters the graph drivers use (reference
// io/data_formatter.h:18-51).  The FPGA layouts of the reference header (CPSR streams, tiled CSC
// packets, :54-721) are produced for CDNA4 inside gl_spmv_plan_create / gl_spmspv_plan_create instead.
#ifndef GRAPHLILY_IO_DATA_FORMATTER_H_
#define GRAPHLILY_IO_DATA_FORMATTER_H_

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "graphlily/global.h"
#include "graphlily/io/data_loader.h"

namespace graphlily {
namespace io {

// Pad rows (empty) and columns up to the next multiple of the divisors, in place.
template <typename data_type>
void util_round_csr_matrix_dim(CSRMatrix<data_type> &m, uint32_t row_divisor, uint32_t col_divisor) {
    if (m.num_rows % row_divisor != 0) {
        const uint32_t pad = row_divisor - m.num_rows % row_divisor;
        m.adj_indptr.insert(m.adj_indptr.end(), pad, m.adj_indptr[m.num_rows]);
        m.num_rows += pad;
    }
    if (m.num_cols % col_divisor != 0) m.num_cols += col_divisor - m.num_cols % col_divisor;
}

// adj_data[i] = 1.0 / (non-zeros in the column of i): double divide, stored as data_type.
template <typename data_type>
void util_normalize_csr_matrix_by_outdegree(CSRMatrix<data_type> &m) {
    if (std::is_same<data_type, float>::value) {   // natively (GPU when the runtime is up): same double divide, float store
        GRAPHLILY_CHECK(gl_csr_normalize_by_outdegree(m.num_rows, m.num_cols, m.adj_indptr.data(), m.adj_indices.data(),
                                                      reinterpret_cast<float *>(m.adj_data.data())));
        return;
    }
    std::vector<uint32_t> per_col(m.num_cols, 0);
    for (uint32_t c : m.adj_indices) per_col[c]++;
    const size_t nnz = m.adj_indptr[m.num_rows];
    for (size_t i = 0; i < nnz; i++) m.adj_data[i] = 1.0 / per_col[m.adj_indices[i]];
}

// The matrix preparation of app::TriangleCount (an extension): the undirected simple graph of m -- an edge {u, v} iff u != v and
// a stored non-zero entry A[v,u] or A[u,v] exists -- oriented by degree.  Row v of the result keeps exactly the neighbours u
// with (deg[u], u) > (deg[v], v), columns ascending, every value 1; `degrees` receives the undirected degrees.  Every triangle
// then appears once in gl_tc_count's set formula and a hub's row is short.  n = max(num_rows, num_cols); apply after padding.
template <typename data_type>
CSRMatrix<data_type> util_triangle_orient(CSRMatrix<data_type> const &m, std::vector<uint32_t> &degrees) {
    const uint64_t n = std::max(m.num_rows, m.num_cols);
    std::vector<uint64_t> key;
    key.reserve(2 * (size_t)m.adj_indptr[m.num_rows]);
    for (uint32_t v = 0; v < m.num_rows; v++)
        for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1]; i++) {
            const uint64_t u = m.adj_indices[i];
            if (u == v || m.adj_data[i] == data_type(0)) continue;
            key.push_back(v * n + u);
            key.push_back(u * n + v);
        }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    degrees.assign(n, 0);
    for (uint64_t k : key) degrees[k / n]++;
    CSRMatrix<data_type> out;
    out.num_rows = out.num_cols = (uint32_t)n;
    out.adj_indptr.assign(n + 1, 0);
    for (uint64_t k : key) {      // (sorted by (row, column): the kept columns of a row ascend)
        const uint64_t a = k / n, b = k % n;
        if (degrees[b] > degrees[a] || (degrees[b] == degrees[a] && b > a)) {
            out.adj_indices.push_back((uint32_t)b);
            out.adj_indptr[a + 1]++;
        }
    }
    for (uint64_t v = 0; v < n; v++) out.adj_indptr[v + 1] += out.adj_indptr[v];
    out.adj_data.assign(out.adj_indices.size(), data_type(1));
    return out;
}

// The matrix preparation of app::KCore (an extension): the undirected simple graph of m -- an edge {u, v} iff u != v and a
// stored non-zero entry A[v,u] or A[u,v] exists -- stored in BOTH directions, once each: row v of the result lists the
// neighbours of v, columns ascending, every value 1; `degrees` receives the row lengths.  n = max(num_rows, num_cols); apply
// after padding.
template <typename data_type>
CSRMatrix<data_type> util_symmetrize_simple(CSRMatrix<data_type> const &m, std::vector<uint32_t> &degrees) {
    const uint64_t n = std::max(m.num_rows, m.num_cols);
    std::vector<uint64_t> key;
    key.reserve(2 * (size_t)m.adj_indptr[m.num_rows]);
    for (uint32_t v = 0; v < m.num_rows; v++)
        for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1]; i++) {
            const uint64_t u = m.adj_indices[i];
            if (u == v || m.adj_data[i] == data_type(0)) continue;
            key.push_back(v * n + u);
            key.push_back(u * n + v);
        }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    if (key.size() > 0xffffffffull) {
        printf("util_symmetrize_simple: %zu entries do not fit 32-bit offsets\n", key.size());
        exit(EXIT_FAILURE);
    }
    degrees.assign(n, 0);
    CSRMatrix<data_type> out;
    out.num_rows = out.num_cols = (uint32_t)n;
    out.adj_indptr.assign(n + 1, 0);
    out.adj_indices.reserve(key.size());
    for (uint64_t k : key) {      // (sorted by (row, column): the columns of a row ascend)
        degrees[k / n]++;
        out.adj_indices.push_back((uint32_t)(k % n));
    }
    for (uint64_t v = 0; v < n; v++) out.adj_indptr[v + 1] = out.adj_indptr[v] + degrees[v];
    out.adj_data.assign(out.adj_indices.size(), data_type(1));
    return out;
}

// The matrix preparation of app::MinimumSpanningForest (an extension): util_symmetrize_simple's layout with weights.  The diagonal
// is dropped; every remaining STORED entry is an edge {u, v}, a stored 0 included.  An edge stored more than once, or in both
// directions, gets the SMALLEST of its values (keep_largest: the LARGEST, io.symmetrize_weighted's keep="largest", the natural
// reading for a maximum-weight result such as app::Matching's), and both entries of the result carry it; -0.0 becomes +0.0; a
// NaN prints and exits.  weighted = false is util_symmetrize_simple's reading (zero values are no edges, every weight 1).  `degrees` receives the
// row lengths.  n = max(num_rows, num_cols); apply after padding.
template <typename data_type>
CSRMatrix<data_type> util_symmetrize_weighted(CSRMatrix<data_type> const &m, std::vector<uint32_t> &degrees, bool weighted = true,
                                              bool keep_largest = false) {
    if (!weighted) return util_symmetrize_simple(m, degrees);
    const uint64_t n = std::max(m.num_rows, m.num_cols);
    std::vector<std::pair<uint64_t, data_type>> edge;          // {lo * n + hi, weight}
    edge.reserve((size_t)m.adj_indptr[m.num_rows]);
    for (uint32_t v = 0; v < m.num_rows; v++)
        for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1]; i++) {
            const uint64_t u = m.adj_indices[i];
            if (u == v) continue;
            const data_type w = m.adj_data[i] + data_type(0);   // (-0.0 + 0.0 == +0.0)
            if (w != w) {
                printf("util_symmetrize_weighted: entry %u (%u, %u) is NaN: the order of the edges needs comparable weights\n", i, v, (uint32_t)u);
                exit(EXIT_FAILURE);
            }
            edge.push_back(std::make_pair(std::min<uint64_t>(u, v) * n + std::max<uint64_t>(u, v), w));
        }
    std::sort(edge.begin(), edge.end());                        // by edge, the smallest value of each first
    if (keep_largest)                                           // ... the largest of each run moves to the run's front
        for (size_t i = 0, j; i < edge.size(); i = j) {
            for (j = i + 1; j < edge.size() && edge[j].first == edge[i].first; j++) {}
            edge[i].second = edge[j - 1].second;
        }
    std::vector<std::pair<uint64_t, data_type>> entry;          // {row * n + column, weight}, both directions
    entry.reserve(2 * edge.size());
    for (size_t i = 0; i < edge.size(); i++) {
        if (i != 0 && edge[i].first == edge[i - 1].first) continue;
        const uint64_t lo = edge[i].first / n, hi = edge[i].first % n;
        entry.push_back(std::make_pair(lo * n + hi, edge[i].second));
        entry.push_back(std::make_pair(hi * n + lo, edge[i].second));
    }
    std::sort(entry.begin(), entry.end());
    if (entry.size() > 0xffffffffull) {
        printf("util_symmetrize_weighted: %zu entries do not fit 32-bit offsets\n", entry.size());
        exit(EXIT_FAILURE);
    }
    degrees.assign(n, 0);
    CSRMatrix<data_type> out;
    out.num_rows = out.num_cols = (uint32_t)n;
    out.adj_indptr.assign(n + 1, 0);
    out.adj_indices.reserve(entry.size());
    out.adj_data.reserve(entry.size());
    for (size_t i = 0; i < entry.size(); i++) {                 // (sorted by (row, column): the columns of a row ascend)
        degrees[entry[i].first / n]++;
        out.adj_indices.push_back((uint32_t)(entry[i].first % n));
        out.adj_data.push_back(entry[i].second);
    }
    for (uint64_t v = 0; v < n; v++) out.adj_indptr[v + 1] = out.adj_indptr[v] + degrees[v];
    return out;
}

// murmur3's fmix32 of (v + 0x9e3779b9 * (seed + 1)) mod 2^32, all arithmetic mod 2^32: a bijection of the 32-bit words, so the
// hashes of distinct vertices never tie (io.coloring_hash computes the same word)
inline uint32_t util_coloring_hash(uint32_t v, uint32_t seed) {
    uint32_t h = v + 0x9e3779b9u * (seed + 1u);
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// The priorities of app::GraphColoring (an extension) for the degrees.size() vertices, the words io.coloring_priorities gives: a
// vertex of larger priority is coloured first, ties go to the smaller vertex number.  "natural": an EMPTY vector (every priority
// equal, plain ascending vertex order); "random": the hash; "largest_first": (min(deg, 4095) << 20) | (hash >> 12);
// "smallest_last": prio[peel_order[i]] = i for the peeling order gl_kcore returns on the same graph -- the last vertex peeled is
// coloured first, and degeneracy + 1 colours suffice.
inline std::vector<uint32_t> util_coloring_priorities(std::vector<uint32_t> const &degrees, std::string const &order, uint32_t seed,
                                                      std::vector<uint32_t> const &peel_order = std::vector<uint32_t>()) {
    const size_t n = degrees.size();
    std::vector<uint32_t> prio;
    if (order == "natural") return prio;
    prio.assign(n, 0);
    if (order == "random") {
        for (size_t v = 0; v < n; v++) prio[v] = util_coloring_hash((uint32_t)v, seed);
    } else if (order == "largest_first") {
        for (size_t v = 0; v < n; v++) prio[v] = (std::min<uint32_t>(degrees[v], 4095u) << 20) | (util_coloring_hash((uint32_t)v, seed) >> 12);
    } else if (order == "smallest_last") {
        if (peel_order.size() != n) {
            printf("util_coloring_priorities: \"smallest_last\" needs the %zu vertices in gl_kcore's peeling order\n", n);
            exit(EXIT_FAILURE);
        }
        for (size_t i = 0; i < n; i++) prio[peel_order[i]] = (uint32_t)i;
    } else {
        printf("util_coloring_priorities: order \"%s\" is none of natural, random, largest_first, smallest_last\n", order.c_str());
        exit(EXIT_FAILURE);
    }
    return prio;
}

// The seeded initial labels of app::LabelPropagation (an extension), io.lpa_initial_labels's words: a permutation of 0 .. n - 1
// over the first n vertices -- label[v] = the rank of util_coloring_hash(v, seed) among them -- and every later (padding) vertex's
// own number.
inline std::vector<uint32_t> util_lpa_initial_labels(uint32_t n, uint32_t seed, uint32_t n_total) {
    std::vector<std::pair<uint32_t, uint32_t>> key(n);
    for (uint32_t v = 0; v < n; v++) key[v] = std::make_pair(util_coloring_hash(v, seed), v);
    std::sort(key.begin(), key.end());
    std::vector<uint32_t> out(std::max(n, n_total));
    for (uint32_t v = 0; v < out.size(); v++) out[v] = v;
    for (uint32_t i = 0; i < n; i++) out[key[i].second] = i;
    return out;
}

// The aggregation step of app::Louvain (an extension), io.aggregate_communities's words: `graph` is a symmetric matrix in
// util_symmetrize_simple's layout (a diagonal entry is ignored), `weights` its integer entry weights (empty: all 1), `k` the vertex
// weights and `labels` one community label per vertex.  The communities are numbered 0 .. count - 1 in ascending order of their
// labels; community_of[v] is the number of v's.  The result has an entry (a, b), a != b, iff an entry joins a member of a to a
// member of b; out_weights holds the SUM of those entries' weights, out_k[a] the sum of k[v] over the members of a (the weight
// inside a community goes there only: the result has no diagonal).
template <typename data_type>
CSRMatrix<data_type> util_aggregate_communities(CSRMatrix<data_type> const &graph, std::vector<uint32_t> const &weights,
                                                std::vector<uint32_t> const &k, std::vector<uint32_t> const &labels,
                                                std::vector<uint32_t> &out_weights, std::vector<uint32_t> &out_k,
                                                std::vector<uint32_t> &community_of) {
    const size_t n = graph.num_rows;
    std::vector<uint32_t> sorted(labels.begin(), labels.begin() + n);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    const uint64_t count = sorted.size();
    community_of.assign(n, 0);
    std::vector<uint64_t> tot(count, 0);
    for (size_t v = 0; v < n; v++) {
        community_of[v] = (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), labels[v]) - sorted.begin());
        tot[community_of[v]] += k[v];
    }
    std::vector<std::pair<uint64_t, uint64_t>> entry;     // (a * count + b, weight)
    for (size_t v = 0; v < n; v++)
        for (uint32_t j = graph.adj_indptr[v]; j < graph.adj_indptr[v + 1]; j++) {
            const uint32_t u = graph.adj_indices[j];
            if (u == v || community_of[u] == community_of[v]) continue;
            entry.push_back(std::make_pair(community_of[v] * count + community_of[u], (uint64_t)(weights.empty() ? 1u : weights[j])));
        }
    std::sort(entry.begin(), entry.end());
    CSRMatrix<data_type> out;
    out.num_rows = out.num_cols = (uint32_t)count;
    out.adj_indptr.assign(count + 1, 0);
    out_weights.clear();
    out_k.assign(count, 0);
    std::vector<uint64_t> sums;
    for (size_t i = 0; i < entry.size(); i++) {
        if (i == 0 || entry[i].first != entry[i - 1].first) {
            out.adj_indices.push_back((uint32_t)(entry[i].first % count));
            out.adj_indptr[entry[i].first / count + 1]++;
            sums.push_back(0);
        }
        sums.back() += entry[i].second;
    }
    for (uint64_t a = 0; a < count; a++) out.adj_indptr[a + 1] += out.adj_indptr[a];
    for (uint64_t a = 0; a < count; a++) {
        if (tot[a] > 0xffffffffull) { printf("util_aggregate_communities: a summed weight does not fit 32 bits\n"); exit(EXIT_FAILURE); }
        out_k[a] = (uint32_t)tot[a];
    }
    for (uint64_t x : sums) {
        if (x > 0xffffffffull) { printf("util_aggregate_communities: a summed weight does not fit 32 bits\n"); exit(EXIT_FAILURE); }
        out_weights.push_back((uint32_t)x);
    }
    out.adj_data.assign(out.adj_indices.size(), data_type(1));
    return out;
}

// The matrix preparation of app::BetweennessCentrality (an extension): the simple DIRECTED graph of m -- an edge u -> v iff u != v
// and a stored non-zero entry A[v,u] exists: zero values, the diagonal and duplicates are dropped, the direction is kept.  Row v of
// `in` lists the vertices v is pulled from, row u of `out` (the transposed pattern) the out-neighbours of u; both n x n, n =
// max(num_rows, num_cols), every value 1, columns ascending.  Returns whether the two are the same matrix (`out` is then left
// empty, 0 x 0).  Apply after padding.
template <typename data_type>
bool util_simple_pattern(CSRMatrix<data_type> const &m, CSRMatrix<data_type> &in, CSRMatrix<data_type> &out) {
    const uint64_t n = std::max(m.num_rows, m.num_cols);
    std::vector<uint64_t> key_in, key_out;
    key_in.reserve(m.adj_indptr[m.num_rows]);
    for (uint32_t v = 0; v < m.num_rows; v++)
        for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1]; i++) {
            const uint64_t u = m.adj_indices[i];
            if (u == v || m.adj_data[i] == data_type(0)) continue;
            key_in.push_back(v * n + u);
        }
    std::sort(key_in.begin(), key_in.end());
    key_in.erase(std::unique(key_in.begin(), key_in.end()), key_in.end());
    key_out.reserve(key_in.size());
    for (uint64_t k : key_in) key_out.push_back(k % n * n + k / n);
    std::sort(key_out.begin(), key_out.end());
    auto build = [n](const std::vector<uint64_t> &key, CSRMatrix<data_type> &r) {      // (sorted by (row, column), once each)
        r.num_rows = r.num_cols = (uint32_t)n;
        r.adj_indptr.assign(n + 1, 0);
        r.adj_indices.clear();
        r.adj_indices.reserve(key.size());
        for (uint64_t k : key) {
            r.adj_indptr[k / n + 1]++;
            r.adj_indices.push_back((uint32_t)(k % n));
        }
        for (uint64_t v = 0; v < n; v++) r.adj_indptr[v + 1] += r.adj_indptr[v];
        r.adj_data.assign(r.adj_indices.size(), data_type(1));
    };
    build(key_in, in);
    const bool symmetric = key_in == key_out;
    out = CSRMatrix<data_type>();
    out.num_rows = out.num_cols = 0;
    if (!symmetric) build(key_out, out);
    return symmetric;
}

// The matrix preparation of app::TopologicalOrder (an extension), io.directed_weighted's words: util_simple_pattern's reading with
// weights.  The diagonal is dropped; every other STORED entry A[v,u] is an edge u -> v, a stored 0 included; an edge stored more
// than once gets its LARGEST value; -0.0 becomes +0.0; a NaN or an infinity prints and exits.  Row v of `in` lists the
// predecessors of v, row u of `out` (the transposed pattern) the successors of u, each with the edge's weight in adj_data; both n
// x n, n = max(num_rows, num_cols), columns ascending.  Returns whether the two PATTERNS are the same; `out` is filled even then
// (its weights are the transposed ones).  weighted = false is util_simple_pattern itself.  Apply after padding.
template <typename data_type>
bool util_directed_weighted(CSRMatrix<data_type> const &m, CSRMatrix<data_type> &in, CSRMatrix<data_type> &out, bool weighted = true) {
    if (!weighted) return util_simple_pattern(m, in, out);
    const uint64_t n = std::max(m.num_rows, m.num_cols);
    std::vector<std::pair<uint64_t, data_type>> entry;          // {row * n + column, weight}
    entry.reserve((size_t)m.adj_indptr[m.num_rows]);
    for (uint32_t v = 0; v < m.num_rows; v++)
        for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1]; i++) {
            const uint64_t u = m.adj_indices[i];
            if (u == v) continue;
            const data_type w = m.adj_data[i] + data_type(0);   // (-0.0 + 0.0 == +0.0)
            if (w != w || w - w != data_type(0)) {
                printf("util_directed_weighted: entry %u (%u, %u) is %g: a longest path needs finite weights\n", i, v, (uint32_t)u, (double)w);
                exit(EXIT_FAILURE);
            }
            entry.push_back(std::make_pair(v * n + u, w));
        }
    std::sort(entry.begin(), entry.end());                      // by entry, the largest value of each last
    std::vector<std::pair<uint64_t, data_type>> once, back;
    for (size_t i = 0; i < entry.size(); i++)
        if (i + 1 == entry.size() || entry[i + 1].first != entry[i].first) once.push_back(entry[i]);
    back.reserve(once.size());
    for (auto const &e : once) back.push_back(std::make_pair(e.first % n * n + e.first / n, e.second));
    std::sort(back.begin(), back.end());
    auto build = [n](const std::vector<std::pair<uint64_t, data_type>> &es, CSRMatrix<data_type> &r) {
        r.num_rows = r.num_cols = (uint32_t)n;
        r.adj_indptr.assign(n + 1, 0);
        r.adj_indices.clear();
        r.adj_data.clear();
        for (auto const &e : es) {
            r.adj_indptr[e.first / n + 1]++;
            r.adj_indices.push_back((uint32_t)(e.first % n));
            r.adj_data.push_back(e.second);
        }
        for (uint64_t v = 0; v < n; v++) r.adj_indptr[v + 1] += r.adj_indptr[v];
    };
    build(once, in);
    build(back, out);
    bool symmetric = true;
    for (size_t i = 0; i < once.size() && symmetric; i++) symmetric = once[i].first == back[i].first;
    return symmetric;
}

}  // namespace io
}  // namespace graphlily

#endif  // GRAPHLILY_IO_DATA_FORMATTER_H_
