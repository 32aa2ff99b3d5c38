"""Host-side matrix containers and formatters of the graphlily::io namespace.

Mirrors (names, argument meaning, in-place behaviour):
  CSRMatrix / CSCMatrix / create_csr_matrix      io/data_loader.h:18-47, 92-104
  load_csr_matrix_from_float_npz                 io/data_loader.h:51-70   (npz parsing done natively by
                                                 gl_npz_csr_* in libgraphlily_hip.so, replacing cnpy)
  csr2csc                                        io/data_loader.h:108-144
  util_round_csr_matrix_dim                      io/data_formatter.h:18-33
  util_normalize_csr_matrix_by_outdegree         io/data_formatter.h:36-51
  triangle_orient                                io/data_formatter.h (util_triangle_orient: an extension, no reference counterpart)
  symmetrize_simple                              io/data_formatter.h (util_symmetrize_simple: an extension, no reference counterpart)
  symmetrize_weighted                            io/data_formatter.h (util_symmetrize_weighted: an extension, no reference counterpart)
  simple_pattern                                 io/data_formatter.h (util_simple_pattern: an extension, no reference counterpart)
  directed_weighted                              io/data_formatter.h (util_directed_weighted: an extension, no reference counterpart)
The FPGA-only formatters (csr2cpsr, formatCSC: io/data_formatter.h:54-721) have no counterpart here:
the device layout is produced inside gl_spmv_plan_create / gl_spmspv_plan_create.
"""
import numpy as np

from . import capi


class CSRMatrix:
    """num_rows, num_cols, adj_data[nnz] f32, adj_indices[nnz] u32, adj_indptr[num_rows+1] u32."""

    def __init__(self, num_rows=0, num_cols=0, adj_data=(), adj_indices=(), adj_indptr=(0,)):
        self.num_rows = int(num_rows)
        self.num_cols = int(num_cols)
        self.adj_data = np.ascontiguousarray(adj_data, dtype=np.float32)
        self.adj_indices = np.ascontiguousarray(adj_indices, dtype=np.uint32)
        self.adj_indptr = np.ascontiguousarray(adj_indptr, dtype=np.uint32)

    @property
    def nnz(self):
        return int(self.adj_indptr[-1])

    def copy(self):
        return type(self)(self.num_rows, self.num_cols, self.adj_data.copy(), self.adj_indices.copy(),
                          self.adj_indptr.copy())


class CSCMatrix(CSRMatrix):
    """Same fields; adj_indices are row ids and adj_indptr has num_cols+1 entries."""


def create_csr_matrix(num_rows, num_cols, adj_data, adj_indices, adj_indptr):
    return CSRMatrix(num_rows, num_cols, adj_data, adj_indices, adj_indptr)


def load_csr_matrix_from_float_npz(csr_float_npz_path):
    nr, nc, data, indices, indptr = capi.npz_load_csr(csr_float_npz_path)
    return CSRMatrix(nr, nc, data, indices, indptr)


def csr2csc(csr_matrix):
    """Transpose (io/data_loader.h:108-144); rows inside a column stay ascending.  Done natively
    (gl_csr2csc: a radix sort on the GPU for large matrices, a parallel counting sort on the host otherwise): the numpy formulation took 18 s on 212 M non-zeros."""
    indptr, indices, data = capi.host_csr2csc(csr_matrix.num_rows, csr_matrix.num_cols, csr_matrix.adj_indptr,
                                              csr_matrix.adj_indices, csr_matrix.adj_data)
    return CSCMatrix(csr_matrix.num_rows, csr_matrix.num_cols, data, indices, indptr)


def util_round_csr_matrix_dim(csr_matrix, row_divisor, col_divisor):
    """Pads in place: extra rows are empty (indptr repeats its last value), extra columns just widen."""
    rem = csr_matrix.num_rows % row_divisor
    if rem:
        pad = row_divisor - rem
        last = csr_matrix.adj_indptr[csr_matrix.num_rows]
        csr_matrix.adj_indptr = np.concatenate([csr_matrix.adj_indptr, np.full(pad, last, dtype=np.uint32)])
        csr_matrix.num_rows += pad
    rem = csr_matrix.num_cols % col_divisor
    if rem:
        csr_matrix.num_cols += col_divisor - rem


def util_normalize_csr_matrix_by_outdegree(csr_matrix):
    """adj_data[i] = 1.0 / (#non-zeros in column of i): double divide, float store."""
    csr_matrix.adj_data = capi.csr_normalize_by_outdegree(csr_matrix.num_rows, csr_matrix.num_cols, csr_matrix.adj_indptr,
                                                          csr_matrix.adj_indices)


def triangle_orient(csr_matrix):
    """The matrix preparation of TriangleCount (an extension) -> (oriented CSRMatrix with every value 1, undirected degrees as
    uint32[n]), n = max(num_rows, num_cols).  The undirected simple graph of the matrix has an edge {u, v} iff u != v and a stored
    non-zero entry A[v, u] or A[u, v] exists: zero values and the diagonal are dropped, the rest is symmetrised and deduplicated;
    deg[v] = neighbours of v in that graph.  Row v of the result keeps exactly the neighbours u with (deg[u], u) > (deg[v], v),
    columns ascending: an acyclic orientation, so every triangle appears once in gl_tc_count's set formula, and a hub's row
    becomes short (at most about sqrt(2 m) entries).  Applied after padding: padding vertices have empty rows."""
    n = max(int(csr_matrix.num_rows), int(csr_matrix.num_cols))
    indptr = csr_matrix.adj_indptr.astype(np.int64)[:csr_matrix.num_rows + 1]
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(csr_matrix.num_rows, dtype=np.int64), np.diff(indptr))
    cols = csr_matrix.adj_indices[:nnz].astype(np.int64)
    keep = (np.asarray(csr_matrix.adj_data[:nnz]) != 0) & (rows != cols)
    rows, cols = rows[keep], cols[keep]
    key = np.unique(np.concatenate([rows * n + cols, cols * n + rows]))       # both directions, once each, sorted by (row, column)
    a, b = key // n, key % n
    deg = np.bincount(a, minlength=n).astype(np.int64)
    up = (deg[b] > deg[a]) | ((deg[b] == deg[a]) & (b > a))
    a, b = a[up], b[up]                                                       # (still sorted: columns ascend inside a row)
    out_indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=out_indptr[1:])
    if int(out_indptr[n]) > 0xFFFFFFFF:
        raise ValueError("triangle_orient: %d entries do not fit 32-bit offsets" % int(out_indptr[n]))
    oriented = CSRMatrix(n, n, np.ones(b.shape[0], dtype=np.float32), b.astype(np.uint32), out_indptr.astype(np.uint32))
    return oriented, deg.astype(np.uint32)


def symmetrize_simple(csr_matrix):
    """The matrix preparation of KCore (an extension) -> (symmetric CSRMatrix with every value 1, degrees as uint32[n]),
    n = max(num_rows, num_cols).  The undirected simple graph of the matrix has an edge {u, v} iff u != v and a stored non-zero
    entry A[v, u] or A[u, v] exists: zero values and the diagonal are dropped, the rest is kept in BOTH directions, once each.
    Row v of the result lists the neighbours of v, columns ascending -- the strictly ascending sets with a symmetric pattern
    that gl_kcore asks for -- and deg[v] is its length.  Applied after padding: padding vertices have empty rows."""
    n = max(int(csr_matrix.num_rows), int(csr_matrix.num_cols))
    indptr = csr_matrix.adj_indptr.astype(np.int64)[:csr_matrix.num_rows + 1]
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(csr_matrix.num_rows, dtype=np.int64), np.diff(indptr))
    cols = csr_matrix.adj_indices[:nnz].astype(np.int64)
    keep = (np.asarray(csr_matrix.adj_data[:nnz]) != 0) & (rows != cols)
    rows, cols = rows[keep], cols[keep]
    key = np.unique(np.concatenate([rows * n + cols, cols * n + rows]))       # both directions, once each, sorted by (row, column)
    a, b = key // n, key % n
    deg = np.bincount(a, minlength=n).astype(np.int64)
    out_indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=out_indptr[1:])
    if int(out_indptr[n]) > 0xFFFFFFFF:
        raise ValueError("symmetrize_simple: %d entries do not fit 32-bit offsets" % int(out_indptr[n]))
    sym = CSRMatrix(n, n, np.ones(b.shape[0], dtype=np.float32), b.astype(np.uint32), out_indptr.astype(np.uint32))
    return sym, deg.astype(np.uint32)


def symmetrize_weighted(csr_matrix, weighted=True, keep="smallest"):
    """The matrix preparation of MinimumSpanningForest (an extension) -> (symmetric CSRMatrix, degrees as uint32[n]),
    n = max(num_rows, num_cols): symmetrize_simple's layout with weights.  The diagonal is dropped; every remaining STORED entry
    is an edge {u, v}, a stored 0 included (weight 0 is a legitimate weight).  An edge stored more than once, or in both
    directions, gets the SMALLEST of its values (keep="largest": the LARGEST, the natural reading for a maximum-weight result such
    as Matching's), and both entries of the result carry it.  -0.0 becomes +0.0; a NaN raises
    ValueError naming the first offending entry.  Row v of the result lists the neighbours of v, columns ascending, with the
    weights in adj_data.  weighted=False is symmetrize_simple's reading: zero values are no edges and every weight is 1.
    Applied after padding: padding vertices have empty rows."""
    if keep not in ("smallest", "largest"):
        raise ValueError("symmetrize_weighted: keep is %r, not \"smallest\" or \"largest\"" % (keep,))
    if not weighted:
        return symmetrize_simple(csr_matrix)
    n = max(int(csr_matrix.num_rows), int(csr_matrix.num_cols))
    indptr = csr_matrix.adj_indptr.astype(np.int64)[:csr_matrix.num_rows + 1]
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(csr_matrix.num_rows, dtype=np.int64), np.diff(indptr))
    cols = csr_matrix.adj_indices[:nnz].astype(np.int64)
    w = np.asarray(csr_matrix.adj_data[:nnz], dtype=np.float32)
    bad = np.isnan(w) & (rows != cols)
    if np.any(bad):
        j = int(np.flatnonzero(bad)[0])
        raise ValueError("symmetrize_weighted: entry %d (%d, %d) is NaN: the order of the edges needs comparable weights" % (j, rows[j], cols[j]))
    off = rows != cols
    rows, cols, w = rows[off], cols[off], w[off] + np.float32(0.0)            # (-0.0 + 0.0 == +0.0)
    key = np.minimum(rows, cols) * n + np.maximum(rows, cols)
    order = np.lexsort((w if keep == "smallest" else -w, key))                # by edge, the value to keep of each first
    key, w = key[order], w[order]
    once = np.ones(key.shape[0], dtype=bool)
    once[1:] = key[1:] != key[:-1]
    key, w = key[once], w[once]
    lo, hi = key // n, key % n
    a, b, w = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w])
    order = np.lexsort((b, a))                                                # both directions, sorted by (row, column)
    a, b, w = a[order], b[order], w[order]
    deg = np.bincount(a, minlength=n).astype(np.int64)
    out_indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=out_indptr[1:])
    if int(out_indptr[n]) > 0xFFFFFFFF:
        raise ValueError("symmetrize_weighted: %d entries do not fit 32-bit offsets" % int(out_indptr[n]))
    sym = CSRMatrix(n, n, w.astype(np.float32), b.astype(np.uint32), out_indptr.astype(np.uint32))
    return sym, deg.astype(np.uint32)


COLORING_ORDERS = ("natural", "random", "largest_first", "smallest_last")


def coloring_hash(v, seed=0):
    """-> uint32 array: murmur3's fmix32 of (v + 0x9e3779b9 * (seed + 1)) mod 2^32, all arithmetic mod 2^32 -- a bijection of the
    32-bit words, so the hashes of distinct vertices never tie"""
    h = (np.asarray(v).astype(np.uint64) + np.uint64(0x9e3779b9) * np.uint64((int(seed) + 1) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def coloring_priorities(degrees, order, seed=0, peel_order=None):
    """The priorities of GraphColoring (an extension) for the len(degrees) vertices -> uint32[n], or None for "natural".  A vertex
    of larger priority is coloured first, ties go to the smaller vertex number (gl_color's order):
      "natural"        None: every priority equal, plain ascending vertex order
      "random"         coloring_hash(v, seed): a permutation, no ties
      "largest_first"  (min(deg[v], 4095) << 20) | (coloring_hash(v, seed) >> 12): by capped degree, then by hash; ties exist
      "smallest_last"  prio[peel_order[i]] = i for the peeling order gl_kcore returns on the same graph: the last vertex
                       peeled is coloured first, every vertex has at most core[v] neighbours before it, so degeneracy + 1
                       colours suffice (Matula & Beck).  The order is not unique: keep the array the run used.
    graphlily::io::util_coloring_priorities (include/graphlily/io/data_formatter.h) computes the same words."""
    deg = np.asarray(degrees)
    n = deg.shape[0]
    if order == "natural":
        return None
    if order == "random":
        return coloring_hash(np.arange(n), seed)
    if order == "largest_first":
        return ((np.minimum(deg.astype(np.uint64), np.uint64(4095)) << np.uint64(20)).astype(np.uint32)
                | (coloring_hash(np.arange(n), seed) >> np.uint32(12)))
    if order == "smallest_last":
        if peel_order is None or np.asarray(peel_order).shape != (n,):
            raise ValueError("coloring_priorities: \"smallest_last\" needs peel_order, the %d vertices in gl_kcore's peeling order" % n)
        prio = np.empty(n, dtype=np.uint32)
        prio[np.asarray(peel_order).astype(np.int64)] = np.arange(n, dtype=np.uint32)
        return prio
    raise ValueError("coloring_priorities: order %r is none of %s" % (order, ", ".join(COLORING_ORDERS)))


def lpa_initial_labels(n, seed, n_total=None):
    """The seeded initial labels of LabelPropagation (an extension) -> uint32[n_total or n]: a permutation of 0 .. n - 1 over the
    first n vertices -- label[v] = the rank of coloring_hash(v, seed) among them; the hash is a bijection, so no two tie -- and
    every later (padding) vertex's own number.  It undoes the pull towards small vertex numbers that the rule's tie-break has.
    graphlily::io::util_lpa_initial_labels (include/graphlily/io/data_formatter.h) computes the same words."""
    total = n if n_total is None else int(n_total)
    out = np.arange(total, dtype=np.uint32)
    out[np.argsort(coloring_hash(np.arange(n), seed), kind="stable")] = np.arange(n, dtype=np.uint32)
    return out


def aggregate_communities(graph, weights, vertex_weights, labels):
    """The aggregation step of Louvain (an extension) -> (community graph, uint32 entry weights, uint32 vertex weights tot,
    community_of as uint32[n]).  `graph` is a symmetric CSRMatrix (symmetrize_simple's layout; a diagonal entry is ignored),
    `weights` its integer entry weights (aligned with adj_indices; None: all 1), `vertex_weights` the k[v] (None: the sums of
    the entry weights) and `labels` one community label per vertex.  The communities are numbered 0 .. k - 1 in ascending
    order of their labels; community_of[v] is the number of v's.  The community graph has an entry (a, b), a != b, iff an
    entry joins a member of a to a member of b, and its weight is the SUM of those entries' weights (parallel edges are
    summed); it has no diagonal: the weight inside a community goes to its vertex weight only, tot[a] = the sum of k[v] over
    the members of a.  So two_m = sum k = sum tot and Q = two_m In - sum tot^2 are the same numbers before and after.
    Vectorised numpy on the host."""
    n = int(graph.num_rows)
    indptr = graph.adj_indptr.astype(np.int64)[:n + 1]
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = graph.adj_indices[:nnz].astype(np.int64)
    w = np.ones(nnz, dtype=np.int64) if weights is None else np.asarray(weights)[:nnz].astype(np.int64)
    off = rows != cols
    rows, cols, w = rows[off], cols[off], w[off]
    if vertex_weights is None:
        k = np.zeros(n, dtype=np.int64)
        np.add.at(k, rows, w)
    else:
        k = np.asarray(vertex_weights).astype(np.int64)
    lab = np.asarray(labels)
    if lab.shape != (n,) or k.shape != (n,):
        raise ValueError("aggregate_communities: %s labels and %s vertex weights for %d vertices" % (lab.shape, k.shape, n))
    _, community_of = np.unique(lab, return_inverse=True)
    community_of = community_of.astype(np.int64).reshape(n)
    kc = int(community_of.max()) + 1 if n else 0
    a, b = community_of[rows], community_of[cols]
    between = a != b
    key, inverse = np.unique(a[between] * kc + b[between], return_inverse=True)      # sorted by (row, column), once each
    wsum = np.zeros(key.shape[0], dtype=np.int64)
    np.add.at(wsum, inverse.reshape(-1), w[between])
    tot = np.zeros(kc, dtype=np.int64)
    np.add.at(tot, community_of, k)
    if (wsum.shape[0] and int(wsum.max()) > 0xFFFFFFFF) or (kc and int(tot.max()) > 0xFFFFFFFF):
        raise ValueError("aggregate_communities: a summed weight does not fit 32 bits")
    out_indptr = np.zeros(kc + 1, dtype=np.int64)
    if kc:
        np.cumsum(np.bincount(key // kc, minlength=kc), out=out_indptr[1:])
    agg = CSRMatrix(kc, kc, np.ones(key.shape[0], dtype=np.float32), (key % max(kc, 1)).astype(np.uint32), out_indptr.astype(np.uint32))
    return agg, wsum.astype(np.uint32), tot.astype(np.uint32), community_of.astype(np.uint32)


def simple_pattern(csr_matrix):
    """The matrix preparation of BetweennessCentrality (an extension) -> (csr_in, csr_out or None, symmetric).  The simple
    directed graph of the matrix has an edge u -> v iff u != v and a stored non-zero entry A[v, u] exists: zero values, the
    diagonal and duplicates are dropped, the direction is KEPT.  Row v of csr_in lists the vertices v is pulled from, row u of
    csr_out (the transposed pattern) the out-neighbours of u; both are n x n, n = max(num_rows, num_cols), every value 1, the
    columns of every row ascending -- the strictly ascending sets gl_bc_accumulate asks for.  `symmetric` says whether the
    two are the same matrix; csr_out is then None.  Applied after padding: padding vertices have empty rows."""
    n = max(int(csr_matrix.num_rows), int(csr_matrix.num_cols))
    indptr = csr_matrix.adj_indptr.astype(np.int64)[:csr_matrix.num_rows + 1]
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(csr_matrix.num_rows, dtype=np.int64), np.diff(indptr))
    cols = csr_matrix.adj_indices[:nnz].astype(np.int64)
    keep = (np.asarray(csr_matrix.adj_data[:nnz]) != 0) & (rows != cols)
    rows, cols = rows[keep], cols[keep]
    if rows.shape[0] > 0xFFFFFFFF:
        raise ValueError("simple_pattern: %d entries do not fit 32-bit offsets" % rows.shape[0])

    def build(key):      # (sorted by (row, column), once each)
        a, b = key // n, key % n
        ip = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(a, minlength=n), out=ip[1:])
        return CSRMatrix(n, n, np.ones(b.shape[0], dtype=np.float32), b.astype(np.uint32), ip.astype(np.uint32))

    key_in, key_out = np.unique(rows * n + cols), np.unique(cols * n + rows)
    symmetric = bool(np.array_equal(key_in, key_out))
    return build(key_in), (None if symmetric else build(key_out)), symmetric


def directed_weighted(csr_matrix, weighted=True):
    """The matrix preparation of TopologicalOrder (an extension) -> (csr_in, csr_out, symmetric): simple_pattern's reading with
    weights.  The diagonal is dropped; every other STORED entry A[v, u] is an edge u -> v, a stored 0 included (weight 0 is a
    legitimate weight); an edge stored more than once gets its LARGEST value (the natural reading for a longest path); -0.0
    becomes +0.0; NaN and +-inf raise ValueError naming the first offending entry.  Row v of csr_in lists the predecessors of
    v, row u of csr_out (the transposed pattern) the successors of u, each with the edge's weight in adj_data; both are n x n,
    n = max(num_rows, num_cols), the columns of every row ascending.  `symmetric` says whether the two PATTERNS are the same;
    csr_out is returned even then, because its weights are the transposed ones.  weighted=False returns exactly what
    simple_pattern returns (zero values are no edges, every value 1, csr_out None for a symmetric pattern).  Applied after
    padding: padding vertices have empty rows."""
    if not weighted:
        return simple_pattern(csr_matrix)
    n = max(int(csr_matrix.num_rows), int(csr_matrix.num_cols))
    indptr = csr_matrix.adj_indptr.astype(np.int64)[:csr_matrix.num_rows + 1]
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(csr_matrix.num_rows, dtype=np.int64), np.diff(indptr))
    cols = csr_matrix.adj_indices[:nnz].astype(np.int64)
    w = np.asarray(csr_matrix.adj_data[:nnz], dtype=np.float32)
    bad = ~np.isfinite(w) & (rows != cols)
    if np.any(bad):
        j = int(np.flatnonzero(bad)[0])
        raise ValueError("directed_weighted: entry %d (%d, %d) is %s: a longest path needs finite weights" % (j, rows[j], cols[j], w[j]))
    off = rows != cols
    rows, cols, w = rows[off], cols[off], w[off] + np.float32(0.0)            # (-0.0 + 0.0 == +0.0)
    if rows.shape[0] > 0xFFFFFFFF:
        raise ValueError("directed_weighted: %d entries do not fit 32-bit offsets" % rows.shape[0])
    key = rows * n + cols
    order = np.lexsort((-w, key))                                             # by entry, the largest value of each first
    key, w = key[order], w[order]
    once = np.ones(key.shape[0], dtype=bool)
    once[1:] = key[1:] != key[:-1]
    key, w = key[once], w[once]

    def build(key, w):      # (sorted by (row, column), once each)
        a, b = key // n, key % n
        ip = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(a, minlength=n), out=ip[1:])
        return CSRMatrix(n, n, w.astype(np.float32), b.astype(np.uint32), ip.astype(np.uint32))

    key_out = key % n * n + key // n
    back = np.argsort(key_out, kind="stable")
    symmetric = bool(np.array_equal(key, key_out[back]))
    return build(key, w), build(key_out[back], w[back]), symmetric


def sssp_add_self_edges(csr_matrix):
    """The matrix preparation of the reference's SSSP app (app/sssp.h:16-62): all weights become 1 and
    weight-0 self edges are added so that a (min,+) SpMV keeps the previous distance.

    The reference edits the CSR arrays in place while walking the rows and reads the end of each
    row from the not-yet-shifted indptr, so after k insertions only the first (len - k) entries of a
    row are examined and rows no longer than k receive no self edge at all.  Results must match the
    reference, so that behaviour is reproduced here rather than "fixed".
    """
    n = csr_matrix.adj_indptr.shape[0] - 1
    indptr = csr_matrix.adj_indptr.astype(np.int64)
    indices = csr_matrix.adj_indices
    lens = np.diff(indptr)
    # rows at or after `r` can only be touched while k <= their length
    suffix_max = np.maximum.accumulate(lens[::-1])[::-1] if n else lens
    insert_at = np.full(n, -1, dtype=np.int64)   # position inside the row where the self edge goes
    zero_at = np.full(n, -1, dtype=np.int64)     # position of an existing diagonal entry to zero
    k = 0
    for r in range(n):
        if k > suffix_max[r]:
            break
        win = int(lens[r]) - k
        if win == 0:
            insert_at[r] = 0
            k += 1
        elif win > 0:
            row = indices[indptr[r]:indptr[r] + win]
            hit = np.nonzero(row >= r)[0]
            if hit.size and row[hit[0]] == r:
                zero_at[r] = hit[0]
            else:
                insert_at[r] = hit[0] if hit.size else win - 1
                k += 1
    has_ins = insert_at >= 0
    new_lens = lens + has_ins
    new_indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(new_lens, out=new_indptr[1:])
    total = int(new_indptr[n])
    out_idx = np.empty(total, dtype=np.uint32)
    out_val = np.ones(total, dtype=np.float32)
    # destination of every original entry: shifted by one inside rows after the insertion point
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos_in_row = np.arange(int(indptr[n]), dtype=np.int64) - indptr[row_of]
    shift = (has_ins[row_of] & (pos_in_row >= insert_at[row_of])).astype(np.int64)
    dest = new_indptr[row_of] + pos_in_row + shift
    out_idx[dest] = indices[:int(indptr[n])]
    rows_ins = np.nonzero(has_ins)[0]
    self_pos = new_indptr[rows_ins] + insert_at[rows_ins]
    out_idx[self_pos] = rows_ins.astype(np.uint32)
    out_val[self_pos] = 0.0
    rows_zero = np.nonzero(zero_at >= 0)[0]
    out_val[new_indptr[rows_zero] + zero_at[rows_zero]] = 0.0
    csr_matrix.adj_indptr = new_indptr.astype(np.uint32)
    csr_matrix.adj_indices = out_idx
    csr_matrix.adj_data = out_val


def sssp_zero_diagonal(csr_matrix):
    """The WEIGHTED preparation of SSSP (an extension: SSSP.load_and_format_matrix(weighted=True); sssp_add_self_edges above is
    the reference's, which sets every weight to 1).  Weights are kept, and every one of the num_rows rows ends up with exactly
    one diagonal entry of value 0, so that a (min,+) SpMV keeps the previous distance: an existing diagonal entry is set to 0
    (further duplicates of it are dropped), otherwise the entry is inserted before the row's first column above the diagonal
    -- in ascending position where the row's columns ascend.  In place.  Raises ValueError for a weight that is negative, NaN
    or >= FLOAT_INF (the semiring's "unreached"), and for a matrix with more rows than columns (no diagonal to hold)."""
    n = int(csr_matrix.num_rows)
    if n > csr_matrix.num_cols:
        raise ValueError("sssp_zero_diagonal: %d rows but %d columns: row %d has no diagonal" % (n, csr_matrix.num_cols, csr_matrix.num_cols))
    indptr = csr_matrix.adj_indptr.astype(np.int64)[:n + 1]
    nnz = int(indptr[n])
    cols = csr_matrix.adj_indices[:nnz]
    data = np.asarray(csr_matrix.adj_data[:nnz], dtype=np.float32)
    bad = ~((data >= 0) & (data < np.float32(999999999.0)))          # (NaN fails both comparisons)
    if np.any(bad):
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("sssp_zero_diagonal: entry %d (row %d, column %d) has weight %r: weights must be >= 0 and < FLOAT_INF"
                         % (k, int(np.searchsorted(indptr, k, side="right")) - 1, int(cols[k]), float(data[k])))
    lens = np.diff(indptr)
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    diag = np.flatnonzero(cols == row_of)
    rows_diag, first = np.unique(row_of[diag], return_index=True)    # (row_of ascends: the first hit of every row)
    has = np.zeros(n, dtype=bool)
    has[rows_diag] = True
    keep = np.ones(nnz, dtype=bool)
    keep[diag] = False
    keep[diag[first]] = True
    data = data.copy()
    data[diag[first]] = 0.0
    if not keep.all():
        cols, data, row_of = cols[keep], data[keep], row_of[keep]
        lens = np.bincount(row_of, minlength=n).astype(np.int64)
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=indptr[1:])
    pos_in_row = np.arange(cols.shape[0], dtype=np.int64) - indptr[row_of]
    insert_at = lens.copy()                                          # after the last entry unless a larger column comes first
    above = np.flatnonzero(cols > row_of)
    rows_above, first = np.unique(row_of[above], return_index=True)
    insert_at[rows_above] = pos_in_row[above[first]]
    new_indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens + ~has, out=new_indptr[1:])
    if int(new_indptr[n]) > 0xFFFFFFFF:
        raise ValueError("sssp_zero_diagonal: %d entries do not fit 32-bit offsets" % int(new_indptr[n]))
    out_idx = np.empty(int(new_indptr[n]), dtype=np.uint32)
    out_val = np.empty(int(new_indptr[n]), dtype=np.float32)
    dest = new_indptr[row_of] + pos_in_row + (~has[row_of] & (pos_in_row >= insert_at[row_of]))
    out_idx[dest] = cols
    out_val[dest] = data
    rows_ins = np.flatnonzero(~has)
    out_idx[new_indptr[rows_ins] + insert_at[rows_ins]] = rows_ins.astype(np.uint32)
    out_val[new_indptr[rows_ins] + insert_at[rows_ins]] = 0.0
    csr_matrix.adj_indptr = new_indptr.astype(np.uint32)
    csr_matrix.adj_indices = out_idx
    csr_matrix.adj_data = out_val
