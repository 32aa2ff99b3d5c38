"""BFS / PageRank / SSSP drivers written against the module API (graphlily::app).

Same public surface and the same module call sequences as the reference drivers
  ModuleCollection  app/module_collection.h:13-114
  BFS               app/bfs.h:20-361      (pull :106-126, push :129-157, pull_push :160-219)
  PageRank          app/pagerank.h:17-160 (pull :80-90)
  SSSP              app/sssp.h:70-254     (pull :152-166, push :169-194, pull_push :197-243)
re-expressed for one process per GPU: every driver optionally takes a dist.Comm; the matrix is
then row-sharded (nnz-balanced ranges), the element-wise steps run on the owned slice, and one
all-gather per iteration rebuilds the dense vector.  With comm=None the sequence
of module calls is exactly the reference's.

Differences that do not change results:
  * modules run non-blocking and the driver synchronises only where the host needs a value
    (get_results_nnz, final read-back) -- the reference finishes the queue after every call;
  * the push->pull switch converts the frontier on the device (gl_sparse_to_dense) instead of
    round-tripping through the host (app/bfs.h:196-201);
  * vectors are allocated by the driver and bound into the modules, so the same buffers can be
    handed to the collective.
"""
import collections
import functools
import math
import os
import time

import numpy as np

from . import capi, io
from . import module as M
from .dist import Comm, partition_rows_by_nnz
from .readback import BookKey, ReadbackBook


# BFS's device-resident schedule (BFS._pull_push_bits): what a recorded hipGraph depends on (packed_read_back: the graph holds
# the pack of levels [lo, lo + own) into the page-locked block), and how one call's levels come back (BFS._readback_plan)
GraphKey = collections.namedtuple("GraphKey", "N threshold back pull_only packed_read_back lo own")
ReadbackPlan = collections.namedtuple("ReadbackPlan", "lo hi own pbits can_pack as_bytes streamed in_graph")

NO_PARENT = 0xFFFFFFFF      # BFS.parents(): the vertex has no predecessor (unreached, or an orphan of a non-BFS level array)


def validate_bfs_tree(csr, source, distance, parent, num_iterations=None):
    """Host-side check (numpy) that `parent` is a BFS tree of `csr` -- row v lists the vertices v is pulled from, entries with
    value 0 are no edges -- consistent with the drivers' levels `distance` (1 on the source, 0 = unreached).  Raises ValueError
    naming the first offending vertex; returns the number of reached vertices.  The rules (Graph500's, in the drivers' terms):
      1. the source has level 1 and is its own parent;
      2. a vertex is reached (level >= 1) exactly if it has a parent;
      3. parent[v] -> v is an edge: A[v, parent[v]] != 0;
      4. level[parent[v]] == level[v] - 1;
      5. no edge A[v, u] leads from an EXPANDED vertex u to a vertex v that is unreached or more than one level deeper.  With
         `num_iterations` given, the search stopped there: u was expanded if 1 <= level[u] <= num_iterations (the last level,
         num_iterations + 1, never was); otherwise every reached u was.
    `distance` / `parent` may be longer than the matrix (the drivers pad it): the extra vertices have empty rows."""
    indptr = np.asarray(csr.adj_indptr).astype(np.int64)
    nr = int(csr.num_rows)
    d = np.asarray(distance, dtype=np.float64)
    p = np.asarray(parent).astype(np.int64)
    n = d.shape[0]
    if p.shape[0] != n or n < max(nr, int(csr.num_cols)):
        raise ValueError("validate_bfs_tree: %d levels and %d parents for a %d x %d matrix" % (n, p.shape[0], nr, csr.num_cols))

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    source = int(source)
    if d[source] != 1 or p[source] != source:
        raise ValueError("validate_bfs_tree: source %d has level %g and parent %d (rule 1)" % (source, d[source], p[source]))
    reached, has_parent = d >= 1, p != NO_PARENT
    if np.any(reached != has_parent):
        v = first(reached != has_parent)
        raise ValueError("validate_bfs_tree: vertex %d has level %g and parent %s (rule 2)" % (v, d[v], "none" if p[v] == NO_PARENT else p[v]))
    child = reached.copy()
    child[source] = False
    if np.any(child & ((p < 0) | (p >= n))):
        raise ValueError("validate_bfs_tree: vertex %d has parent %d, which is no vertex (rule 3)" % (first(child & ((p < 0) | (p >= n))), p[first(child & ((p < 0) | (p >= n)))]))
    pc = np.where(child, p, 0)
    if np.any(child & (d[pc] != d - 1)):
        v = first(child & (d[pc] != d - 1))
        raise ValueError("validate_bfs_tree: vertex %d on level %g has parent %d on level %g (rule 4)" % (v, d[v], p[v], d[p[v]]))
    expanded = reached if num_iterations is None else reached & (d <= num_iterations)
    is_edge = np.zeros(n, dtype=bool)
    step = 1 << 18                       # rows per block: bounds the temporaries on matrices of 1e8 entries
    for r0 in range(0, nr, step):
        r1 = min(nr, r0 + step)
        lo, hi = indptr[r0], indptr[r1]
        if hi == lo:
            continue
        cols = np.asarray(csr.adj_indices[lo:hi]).astype(np.int64)
        live = np.asarray(csr.adj_data[lo:hi]) != 0
        rows = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(indptr[r0:r1 + 1]))
        is_edge[rows[live & (cols == p[rows])]] = True
        bad = live & expanded[cols] & ((d[rows] == 0) | (d[rows] > d[cols] + 1))
        if np.any(bad):
            k = first(bad)
            raise ValueError("validate_bfs_tree: edge %d -> %d leads from level %g to level %g (rule 5)"
                             % (cols[k], rows[k], d[cols[k]], d[rows[k]]))
    if np.any(child & ~is_edge):
        v = first(child & ~is_edge)
        raise ValueError("validate_bfs_tree: vertex %d has parent %d, but the matrix has no entry A[%d, %d] (rule 3)" % (v, p[v], v, p[v]))
    return int(reached.sum())


def validate_sssp_tree(csr, source, distance, parent, unreached=M.FLOAT_INF, converged=True):
    """Host-side check (numpy) that `parent` is a shortest-path tree of `csr` -- row v lists the vertices v is pulled from, every
    stored entry is an edge, weight 0 included -- consistent with the distances `distance` (0 on the source, `unreached` where no
    path was found).  All sums are formed in float32, as the (min,+) operators form them.  Raises ValueError naming the first
    offending vertex and the rule; returns the number of reached vertices.  The rules (Graph500's SSSP checks, in the drivers' terms):
      1. the source has distance 0 and is its own parent;
      2. a vertex is reached (d < unreached) exactly if it has a parent;
      3. parent[v] is a vertex, some stored entry A[v, parent[v]] of weight w has (float)(d[p] + w) == d[v], and d[p] < d[v];
      4. with `converged`: no stored entry A[v, u] with u reached has (float)(d[u] + w) < d[v] -- v unreached included.  A run
         that was cut short (too few iterations) is checked with converged=False.
    `distance` / `parent` may be longer than the matrix (the drivers pad it): the extra vertices have empty rows."""
    indptr = np.asarray(csr.adj_indptr).astype(np.int64)
    nr = int(csr.num_rows)
    d = np.asarray(distance, dtype=np.float32)
    p = np.asarray(parent).astype(np.int64)
    n = d.shape[0]
    if p.shape[0] != n or n < max(nr, int(csr.num_cols)):
        raise ValueError("validate_sssp_tree: %d distances and %d parents for a %d x %d matrix" % (n, p.shape[0], nr, csr.num_cols))

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    source = int(source)
    if d[source] != 0 or p[source] != source:
        raise ValueError("validate_sssp_tree: source %d has distance %g and parent %d (rule 1)" % (source, d[source], p[source]))
    reached, has_parent = d < np.float32(unreached), p != NO_PARENT
    if np.any(reached != has_parent):
        v = first(reached != has_parent)
        raise ValueError("validate_sssp_tree: vertex %d has distance %g and parent %s (rule 2)" % (v, d[v], "none" if p[v] == NO_PARENT else p[v]))
    child = reached.copy()
    child[source] = False
    if np.any(child & ((p < 0) | (p >= n))):
        v = first(child & ((p < 0) | (p >= n)))
        raise ValueError("validate_sssp_tree: vertex %d has parent %d, which is no vertex (rule 3)" % (v, p[v]))
    pc = np.where(child, p, 0)
    is_entry = np.zeros(n, dtype=bool)
    tight = np.zeros(n, dtype=bool)
    step = 1 << 18                       # rows per block: bounds the temporaries on matrices of 1e8 entries
    for r0 in range(0, nr, step):
        r1 = min(nr, r0 + step)
        lo, hi = indptr[r0], indptr[r1]
        if hi == lo:
            continue
        cols = np.asarray(csr.adj_indices[lo:hi]).astype(np.int64)
        through = d[cols] + np.asarray(csr.adj_data[lo:hi], dtype=np.float32)      # float32 + float32
        rows = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(indptr[r0:r1 + 1]))
        to_parent = cols == p[rows]
        is_entry[rows[to_parent]] = True
        tight[rows[to_parent & (through == d[rows])]] = True
        if converged:
            bad = reached[cols] & (through < d[rows])
            if np.any(bad):
                k = first(bad)
                raise ValueError("validate_sssp_tree: entry A[%d, %d] gives %d the distance %r, it has %r (rule 4)"
                                 % (rows[k], cols[k], rows[k], float(through[k]), float(d[rows[k]])))
    if np.any(child & ~is_entry):
        v = first(child & ~is_entry)
        raise ValueError("validate_sssp_tree: vertex %d has parent %d, but the matrix has no entry A[%d, %d] (rule 3)" % (v, p[v], v, p[v]))
    if np.any(child & ~tight):
        v = first(child & ~tight)
        raise ValueError("validate_sssp_tree: vertex %d at distance %r has parent %d at %r, and no entry A[%d, %d] makes up the difference (rule 3)"
                         % (v, float(d[v]), p[v], float(d[p[v]]), v, p[v]))
    if np.any(child & ~(d[pc] < d)):
        v = first(child & ~(d[pc] < d))
        raise ValueError("validate_sssp_tree: vertex %d at distance %r has parent %d at distance %r, which is not smaller (rule 3)"
                         % (v, float(d[v]), p[v], float(d[p[v]])))
    return int(reached.sum())


def _components_of(indptr, indices, data, n):
    """Min-vertex labels of the weak components of a CSR over n vertices: a union-find in numpy, whole rounds at a time (kept
    apart from the device's: validate_components checks one with the other).  An entry (v, u) is an edge unless its value is
    0 (data None: every entry counts) or u >= n.  Between rounds lab[v] is the root of v's tree and the smallest vertex in it."""
    indptr = np.asarray(indptr).astype(np.int64)
    nr = indptr.shape[0] - 1
    rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(indptr))
    cols = np.asarray(indices[:indptr[nr]]).astype(np.int64)
    live = (cols < n) & (rows < n)
    if data is not None:
        live &= np.asarray(data[:indptr[nr]]) != 0
    rows, cols = rows[live], cols[live]
    lab = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = lab[rows], lab[cols]
        cross = ra != rb
        if not np.any(cross):
            return lab
        ra, rb = ra[cross], rb[cross]
        nxt = lab.copy()
        np.minimum.at(nxt, np.maximum(ra, rb), np.minimum(ra, rb))      # hook: the larger root under the smaller (trees descend) ...
        while True:                                                     # ... and compress: every vertex to its root
            hop = nxt[nxt]
            if np.array_equal(hop, nxt):
                break
            nxt = hop
        lab = nxt


def validate_components(csr, labels):
    """Host-side check (numpy) that `labels` are the weakly connected components of `csr` -- row v lists the vertices v is pulled
    from, entries with value 0 are no edges, direction is ignored -- each vertex labelled with the SMALLEST vertex of its
    component.  Raises ValueError naming the first offender and the rule; returns the number of components among the vertices
    `labels` covers.  The rules:
      1. labels[labels[v]] == labels[v] and labels[v] <= v;
      2. every stored non-zero entry (v, u) has labels[v] == labels[u];
      3. no two label classes are joined and every class is connected: the classes are exactly the components an independent
         numpy pass finds (with rules 1 and 2 a class is a union of whole components named by its smallest vertex, so what is
         left to refute is a class that falls apart).
    `labels` may be longer than the matrix (the drivers pad it): the extra vertices have empty rows."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    lab = np.asarray(labels).astype(np.int64)
    n = lab.shape[0]
    if lab.ndim != 1 or n < max(nr, nc):
        raise ValueError("validate_components: %d labels for a %d x %d matrix" % (n, nr, nc))

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    v = np.arange(n, dtype=np.int64)
    if np.any((lab < 0) | (lab > v)):
        k = first((lab < 0) | (lab > v))
        raise ValueError("validate_components: vertex %d has label %d, which is above it (rule 1)" % (k, lab[k]))
    if np.any(lab[lab] != lab):
        k = first(lab[lab] != lab)
        raise ValueError("validate_components: vertex %d has label %d, whose own label is %d (rule 1)" % (k, lab[k], lab[lab[k]]))
    indptr = np.asarray(csr.adj_indptr).astype(np.int64)
    step = 1 << 18                       # rows per block: bounds the temporaries on matrices of 1e8 entries
    for r0 in range(0, nr, step):
        r1 = min(nr, r0 + step)
        lo, hi = indptr[r0], indptr[r1]
        if hi == lo:
            continue
        cols = np.asarray(csr.adj_indices[lo:hi]).astype(np.int64)
        live = np.asarray(csr.adj_data[lo:hi]) != 0
        rows = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(indptr[r0:r1 + 1]))
        bad = live & (lab[rows] != lab[cols])
        if np.any(bad):
            k = first(bad)
            raise ValueError("validate_components: entry A[%d, %d] joins label %d and label %d (rule 2)"
                             % (rows[k], cols[k], lab[rows[k]], lab[cols[k]]))
    own = _components_of(indptr, csr.adj_indices, csr.adj_data, n)
    if np.any(own != lab):
        k = first(own != lab)
        raise ValueError("validate_components: vertex %d has label %d, but no chain of entries joins the two: its component's smallest "
                         "vertex is %d (rule 3)" % (k, lab[k], own[k]))
    return int(np.count_nonzero(lab == v))


def validate_triangles(csr, triangles):
    """Host-side check (scipy) that triangles[v] is the number of triangles through v in the undirected simple graph of `csr`
    -- an edge {u, v} iff u != v and a stored non-zero entry A[v, u] or A[u, v] exists; duplicates, the diagonal, zero values and
    direction are ignored.  An independent statement, on the symmetrised pattern S (no orientation): triangles[v] = ((S S) o S)
    row sum / 2.  Raises ValueError naming the first offending vertex and both values; returns the number of triangles.
    `triangles` may be longer than the matrix (the drivers pad it): the extra vertices are in no triangle."""
    import scipy.sparse as sp
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    t = np.asarray(triangles)
    n = t.shape[0] if t.ndim == 1 else -1
    if n < max(nr, nc):
        raise ValueError("validate_triangles: %d counts for a %d x %d matrix" % (n, nr, nc))
    indptr = np.asarray(csr.adj_indptr).astype(np.int64)[:nr + 1]
    nnz = int(indptr[-1])
    A = sp.csr_matrix((np.asarray(csr.adj_data[:nnz]) != 0, np.asarray(csr.adj_indices[:nnz]).astype(np.int64), indptr), shape=(nr, nc))
    A.resize((n, n))
    A.eliminate_zeros()
    S = (A + A.T).tocsr()
    S.setdiag(0)
    S.eliminate_zeros()
    S.data = np.ones(S.nnz, dtype=np.int64)
    twice = np.asarray((S @ S).multiply(S).sum(axis=1)).ravel().astype(np.int64)
    want = twice // 2
    bad = np.flatnonzero(want != t.astype(np.int64))
    if bad.size:
        k = int(bad[0])
        raise ValueError("validate_triangles: vertex %d is given %d triangles, it lies in %d" % (k, int(t[k]), int(want[k])))
    return int(want.sum()) // 3


def _core_numbers_of(indptr, indices, n):
    """Core numbers of a symmetric simple CSR over n vertices: a peel by whole SETS in numpy (kept apart from the device's queue:
    validate_cores checks one with the other).  At level k every live vertex of degree <= k is removed at once, gets core k, and
    the degrees of its neighbours drop by a bincount; when nobody qualifies k jumps to the smallest live degree."""
    indptr = np.asarray(indptr).astype(np.int64)
    indices = np.asarray(indices)
    deg = np.diff(indptr)
    core = np.zeros(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    left, k = n, 0
    while left:
        cand = np.flatnonzero(alive & (deg <= k))
        if cand.size == 0:
            k = int(deg[alive].min())
            continue
        core[cand] = k
        alive[cand] = False
        left -= cand.size
        starts, lens = indptr[cand], indptr[cand + 1] - indptr[cand]
        total = int(lens.sum())
        if total:
            at = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
            deg = deg - np.bincount(indices[at].astype(np.int64), minlength=n)      # (dead vertices' words go on sinking: never read)
    return core


def validate_cores(csr, core, order=None):
    """Host-side check (numpy) that `core` are the core numbers of the undirected simple graph of `csr` -- an edge {u, v} iff
    u != v and a stored non-zero entry A[v, u] or A[u, v] exists; duplicates, the diagonal, zero values and direction are
    ignored -- and, when given, that `order` is a degeneracy ordering.  Raises ValueError naming the first offender and the
    rule; returns the degeneracy.  The rules:
      1. 0 <= core[v] <= deg[v], and at least core[v] neighbours u of v have core[u] >= core[v] (v's core holds together);
      2. the array equals an independent host computation, a peel by whole sets (what is left to refute after rule 1 is a
         value that is too LOW);
      3. order is a permutation of the vertices, core[order[i]] never descends, and every vertex v has at most core[v]
         neighbours behind it in the order.
    `core` and `order` may be longer than the matrix (the drivers pad them): the extra vertices are isolated."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    c = np.asarray(core)
    n = c.shape[0] if c.ndim == 1 else -1
    if n < max(nr, nc):
        raise ValueError("validate_cores: %d core numbers for a %d x %d matrix" % (n, nr, nc))
    c = c.astype(np.int64)
    sym, deg = io.symmetrize_simple(csr)
    m = sym.num_rows
    indptr = np.concatenate([sym.adj_indptr.astype(np.int64), np.full(n - m, sym.nnz, dtype=np.int64)])
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    cols = sym.adj_indices.astype(np.int64)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    if np.any((c < 0) | (c > deg)):
        v = first((c < 0) | (c > deg))
        raise ValueError("validate_cores: vertex %d of degree %d is given core number %d (rule 1)" % (v, deg[v], c[v]))
    support = np.bincount(rows[c[cols] >= c[rows]], minlength=n)
    if np.any(support < c):
        v = first(support < c)
        raise ValueError("validate_cores: vertex %d is given core number %d, but only %d of its neighbours have one that high (rule 1)"
                         % (v, c[v], support[v]))
    own = _core_numbers_of(indptr, cols, n)
    if np.any(own != c):
        v = first(own != c)
        raise ValueError("validate_cores: vertex %d is given core number %d, its core number is %d (rule 2)" % (v, c[v], own[v]))
    if order is not None:
        o = np.asarray(order)
        if o.ndim != 1 or o.shape[0] != n:
            raise ValueError("validate_cores: an order of %d vertices for %d core numbers (rule 3)" % (o.shape[0] if o.ndim == 1 else -1, n))
        o = o.astype(np.int64)
        seen = np.bincount(o[(o >= 0) & (o < n)], minlength=n)
        if np.any((o < 0) | (o >= n)) or np.any(seen != 1):
            v = first((o < 0) | (o >= n)) if np.any((o < 0) | (o >= n)) else first(seen != 1)
            raise ValueError("validate_cores: the order is no permutation: %s (rule 3)"
                             % ("position %d holds %d" % (v, o[v]) if np.any((o < 0) | (o >= n)) else "vertex %d occurs %d times" % (v, seen[v])))
        if np.any(np.diff(c[o]) < 0):
            i = first(np.diff(c[o]) < 0)
            raise ValueError("validate_cores: the order puts vertex %d (core number %d) before vertex %d (core number %d) (rule 3)"
                             % (o[i], c[o[i]], o[i + 1], c[o[i + 1]]))
        pos = np.empty(n, dtype=np.int64)
        pos[o] = np.arange(n, dtype=np.int64)
        behind = np.bincount(rows[pos[cols] > pos[rows]], minlength=n)
        if np.any(behind > c):
            v = first(behind > c)
            raise ValueError("validate_cores: vertex %d with core number %d has %d neighbours behind it in the order (rule 3)"
                             % (v, c[v], behind[v]))
    return int(c.max()) if n else 0


def _first_fit_of(indptr, indices, n, colors, prio):
    """mex[v] = the smallest non-negative integer that is not colors[u] for any entry u of row v that goes before v in gl_color's
    order (prio[u] > prio[v], or equal and u < v; prio None: all equal), for a symmetric simple CSR over n vertices, in numpy.
    colors IS the first-fit greedy colouring of that order iff mex == colors: by induction along the order, every vertex's
    colour is then the one the sequential loop would give it."""
    indptr = np.asarray(indptr).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = np.asarray(indices).astype(np.int64)
    if prio is None:
        before = cols < rows
    else:
        p = np.asarray(prio).astype(np.int64)
        before = (p[cols] > p[rows]) | ((p[cols] == p[rows]) & (cols < rows))
    c = np.asarray(colors).astype(np.int64)
    span = int(c.max()) + 2 if n else 1
    key = np.unique(rows[before] * span + c[cols[before]])             # per vertex, the colours before it, ascending, once each
    kv, kc = key // span, key % span
    first = np.searchsorted(kv, np.arange(n, dtype=np.int64))
    count = np.searchsorted(kv, np.arange(n, dtype=np.int64), side="right") - first
    rank = np.arange(key.shape[0], dtype=np.int64) - first[kv]
    mex = count.copy()                                                   # colours 0 .. count - 1 all taken: the next one
    gap = kc != rank                                                     # the first rank whose colour is not the rank itself
    np.minimum.at(mex, kv[gap], rank[gap])
    return mex


def validate_coloring(csr, colors, priorities=False):
    """Host-side check (numpy) that `colors` is a colouring of the undirected simple graph of `csr` -- an edge {u, v} iff u != v
    and a stored non-zero entry A[v, u] or A[u, v] exists; duplicates, the diagonal, zero values and direction are ignored -- of
    the kind gl_color produces.  Raises ValueError naming the first offender and the rule; returns the number of colours.  The
    rules:
      1. no edge joins two vertices of one colour (the colouring is proper);
      2. 0 <= colors[v] <= deg[v] (first-fit never skips more colours than v has neighbours);
      3. colour class 0 is a MAXIMAL independent set: every vertex outside it has a neighbour inside;
      4. with `priorities` an array (larger first, ties to the smaller vertex number) or None (ascending vertex order): colors[v]
         is the smallest colour that no neighbour going before v has -- the array is exactly the sequential first-fit greedy
         colouring in that order.  The default False skips this rule.
    `colors` and `priorities` may be longer than the matrix (the drivers pad them): the extra vertices are isolated; priorities
    shorter than colors are extended with 0 (an isolated vertex's priority does not matter)."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    c = np.asarray(colors)
    n = c.shape[0] if c.ndim == 1 else -1
    if n < max(nr, nc):
        raise ValueError("validate_coloring: %d colours for a %d x %d matrix" % (n, nr, nc))
    c = c.astype(np.int64)
    sym, deg = io.symmetrize_simple(csr)
    m = sym.num_rows
    indptr = np.concatenate([sym.adj_indptr.astype(np.int64), np.full(n - m, sym.nnz, dtype=np.int64)])
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    cols = sym.adj_indices.astype(np.int64)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    same = c[rows] == c[cols]
    if np.any(same):
        i = first(same)
        raise ValueError("validate_coloring: the neighbours %d and %d both have colour %d (rule 1)" % (rows[i], cols[i], c[rows[i]]))
    if np.any((c < 0) | (c > deg)):
        v = first((c < 0) | (c > deg))
        raise ValueError("validate_coloring: vertex %d of degree %d is given colour %d (rule 2)" % (v, deg[v], c[v]))
    covered = np.bincount(rows[c[cols] == 0], minlength=n) > 0
    if np.any((c != 0) & ~covered):
        v = first((c != 0) & ~covered)
        raise ValueError("validate_coloring: vertex %d of colour %d has no neighbour of colour 0: class 0 is not maximal (rule 3)" % (v, c[v]))
    if priorities is not False:
        prio = None
        if priorities is not None:
            prio = np.asarray(priorities)
            if prio.ndim != 1 or prio.shape[0] < max(nr, nc) or prio.shape[0] > n:
                raise ValueError("validate_coloring: %d priorities for %d colours (rule 4)" % (prio.shape[0] if prio.ndim == 1 else -1, n))
            prio = np.concatenate([prio.astype(np.int64), np.zeros(n - prio.shape[0], dtype=np.int64)])
        want = _first_fit_of(indptr, cols, n, c, prio)
        if np.any(want != c):
            v = first(want != c)
            raise ValueError("validate_coloring: vertex %d is given colour %d, the smallest colour its earlier neighbours leave free is %d "
                             "(rule 4)" % (v, c[v], want[v]))
    return int(c.max()) + 1 if n else 0


def _edges_and_triangles_of(indptr, indices, n, chunk=1 << 22):
    """The edges and the triangles of a symmetric simple CSR over n vertices, in numpy -> (eid as int64[nnz]: the edge of every
    entry, the entries with row < column numbered in row order and -1 on the diagonal; eu, ev: the ends of every edge, eu < ev;
    tri as int64[T, 3]: the edges (u, v), (v, w), (u, w) of every triangle u < v < w, once each).  For every edge (u, v) the
    neighbours w > v of v are looked up among the neighbours of u."""
    indptr = np.asarray(indptr).astype(np.int64)
    cols = np.asarray(indices).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    up = np.flatnonzero(cols > rows)
    eu, ev = rows[up], cols[up]
    m = up.shape[0]
    key = eu * n + ev                                                    # ascending: row order, ascending rows
    eid = np.full(cols.shape[0], -1, dtype=np.int64)
    eid[up] = np.arange(m, dtype=np.int64)
    low = np.flatnonzero(cols < rows)
    eid[low] = np.searchsorted(key, cols[low] * n + rows[low])
    first = np.searchsorted(eu, np.arange(n, dtype=np.int64))           # a vertex's edges to larger neighbours: first, count
    count = np.bincount(eu, minlength=n)
    lens = count[ev]
    ends = np.cumsum(lens)
    found, lo = [], 0
    while lo < m:
        hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + chunk, side="right")))
        ln = lens[lo:hi]
        total = int(ln.sum())
        if total:
            e = np.repeat(np.arange(lo, hi, dtype=np.int64), ln)
            vw = np.repeat(first[ev[lo:hi]] - (np.cumsum(ln) - ln), ln) + np.arange(total, dtype=np.int64)    # the edge (v, w)
            want = eu[e] * n + ev[vw]
            uw = np.minimum(np.searchsorted(key, want), m - 1)
            hit = key[uw] == want
            found.append(np.stack([e[hit], vw[hit], uw[hit]], axis=1))
        lo = hi
    tri = np.concatenate(found) if found else np.zeros((0, 3), dtype=np.int64)
    return eid, eu, ev, tri


def _truss_numbers_of(m, tri):
    """Truss numbers of the m edges of a graph whose triangles are tri (int64[T, 3], edge numbers): a peel by whole SETS in numpy
    (kept apart from the device's queue: validate_truss checks one with the other) -> (truss as int64[m], support as int64[m],
    levels, sub_rounds).  At level l every edge still there whose count of remaining triangles is l is removed at once and gets
    truss l + 2; every triangle that loses an edge takes one from the count of its edges that stay, but never below l; those
    that arrive at l form the next set of the level.  When nobody qualifies l jumps to the smallest remaining count.  levels =
    levels that removed an edge; sub_rounds = the sets removed."""
    T = tri.shape[0]
    support = np.bincount(tri.ravel(), minlength=m).astype(np.int64)
    order = np.argsort(tri.ravel(), kind="stable")                       # the triangles of every edge
    of_edge = order // 3
    begin = np.concatenate([[0], np.cumsum(support)])
    S = support.copy()
    there = np.ones(m, dtype=bool)
    whole = np.ones(T, dtype=bool)
    truss = np.zeros(m, dtype=np.int64)
    left, l, levels, sub_rounds = m, 0, 0, 0
    while left:
        cur = np.flatnonzero(there & (S == l))
        if cur.size == 0:
            l = int(S[there].min())
            continue
        levels += 1
        while cur.size:
            sub_rounds += 1
            there[cur] = False
            truss[cur] = l + 2
            left -= cur.size
            lens = support[cur]
            total = int(lens.sum())
            if total == 0 or left == 0:
                break
            at = np.repeat(begin[cur] - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
            t = np.unique(of_edge[at])
            t = t[whole[t]]
            whole[t] = False
            stay = tri[t].ravel()
            stay = stay[there[stay]]
            S = S - np.bincount(stay, minlength=m)
            hit = np.unique(stay)
            S[hit] = np.maximum(S[hit], l)
            cur = hit[S[hit] == l]
    return truss, support, levels, sub_rounds


def validate_truss(csr, truss, peel=True):
    """Host-side check (numpy) that `truss` are the truss numbers of the undirected simple graph of `csr` -- an edge {u, v} iff
    u != v and a stored non-zero entry A[v, u] or A[u, v] exists; duplicates, the diagonal, zero values and direction are
    ignored -- one value per entry of io.symmetrize_simple(csr)[0], as KTruss.run() returns them.  Raises ValueError naming the
    first offending entry and the rule; returns the largest truss number (0 for a graph without edges).  The rules:
      1. both entries of an edge carry one value, which is at least 2, and every edge e lies in at least truss[e] - 2 triangles
         whose other two edges have truss >= truss[e] (the edges of truss >= k then hold together as a k-truss, so no value is
         too HIGH);
      2. the array equals an independent host computation, a peel by whole sets over the list of triangles (what is left to
         refute after rule 1 is a value that is too LOW); peel=False skips this rule."""
    sym, _ = io.symmetrize_simple(csr)
    t = np.asarray(truss)
    if t.ndim != 1 or t.shape[0] != sym.nnz:
        raise ValueError("validate_truss: %d truss numbers for the %d entries of the symmetric matrix" % (t.shape[0] if t.ndim == 1 else -1, sym.nnz))
    if sym.nnz == 0:
        return 0
    t = t.astype(np.int64)
    n = sym.num_rows
    eid, eu, ev, tri = _edges_and_triangles_of(sym.adj_indptr, sym.adj_indices, n)
    m = eu.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
    cols = sym.adj_indices.astype(np.int64)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    per_edge = np.zeros(m, dtype=np.int64)
    per_edge[eid[cols > rows]] = t[cols > rows]
    if np.any(per_edge[eid] != t):
        j = first(per_edge[eid] != t)
        raise ValueError("validate_truss: entry %d (%d, %d) is given truss %d, its mirror entry %d (rule 1)"
                         % (j, rows[j], cols[j], t[j], per_edge[eid[j]]))
    if np.any(t < 2):
        j = first(t < 2)
        raise ValueError("validate_truss: entry %d (%d, %d) is given truss %d, an edge has at least 2 (rule 1)" % (j, rows[j], cols[j], t[j]))
    floor = per_edge[tri].min(axis=1) if tri.shape[0] else np.zeros(0, dtype=np.int64)   # a triangle serves the edges up to its weakest
    held = np.zeros(m, dtype=np.int64)
    for c in range(3):
        np.add.at(held, tri[:, c], floor >= per_edge[tri[:, c]])
    if np.any(held < per_edge - 2):
        e = first(held < per_edge - 2)
        j = first(eid == e)
        raise ValueError("validate_truss: entry %d (%d, %d) is given truss %d, but only %d of its triangles have two other edges that high "
                         "(rule 1)" % (j, eu[e], ev[e], per_edge[e], held[e]))
    own = _truss_numbers_of(m, tri)[0] if peel else per_edge
    if np.any(own != per_edge):
        e = first(own != per_edge)
        j = first(eid == e)
        raise ValueError("validate_truss: entry %d (%d, %d) is given truss %d, its truss number is %d (rule 2)"
                         % (j, eu[e], ev[e], per_edge[e], own[e]))
    return int(per_edge.max())


def _edge_keys(weights):
    """key(w) of f32 weights as uint32: the monotone map b ^ (b >> 31 ? 0xffffffff : 0x80000000) of the bits b -- gl_msf's order"""
    b = np.ascontiguousarray(weights, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def _kruskal_of(sym):
    """Kruskal's algorithm on a symmetric CSRMatrix with weights in adj_data, the edges taken in gl_msf's order (key(w), lo, hi):
    the entries above the diagonal sorted by (key, entry number), a union-find with path halving on the host (kept apart from the
    device's Boruvka rounds: validate_spanning_forest checks one with the other) -> bool[nnz], both entries of a forest edge
    marked.  Only the weights of entries above the diagonal are read."""
    n = sym.num_rows
    indptr = sym.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = sym.adj_indices.astype(np.int64)
    up = np.flatnonzero(cols > rows)
    up = up[np.argsort(_edge_keys(sym.adj_data[up]), kind="stable")]        # (stable: ties stay in entry order = (lo, hi) order)
    parent = list(range(n))
    taken = []
    for j, u, v in zip(up.tolist(), rows[up].tolist(), cols[up].tolist()):
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        if u != v:
            parent[max(u, v)] = min(u, v)
            taken.append(j)
    mask = np.zeros(sym.nnz, dtype=bool)
    taken = np.asarray(taken, dtype=np.int64)
    mask[taken] = True
    lo, hi = rows[taken], cols[taken]                                       # the mirror entries: (hi, lo) in row hi
    entry_key = rows * n + cols                                             # ascending: rows are sorted sets
    mask[np.searchsorted(entry_key, hi * n + lo)] = True
    return mask


def validate_spanning_forest(csr, in_forest, weighted=True):
    """Host-side check (numpy) that `in_forest` marks THE minimum spanning forest of the undirected weighted graph of `csr` -- as
    io.symmetrize_weighted(csr, weighted) reads it -- one word per entry of that symmetric matrix, as MinimumSpanningForest.run()
    returns them.  Raises ValueError naming the first offending entry and the rule; returns the number of forest edges.  The rules:
      1. both entries of an edge carry the same mark;
      2. the marked edges are acyclic and span every component: joined by marked edges alone the vertices fall into exactly
         n - edges classes (no cycle), and these are the components of the graph (an independent numpy pass finds them);
      3. the forest is minimal, and the unique one under the order (key(w), lo, hi): it equals, as a whole set, what a host
         Kruskal taking the edges in that order returns (by the cycle property a spanning forest that differs from it holds an
         edge that is the largest of a cycle)."""
    sym, _ = io.symmetrize_weighted(csr, weighted)
    f = np.asarray(in_forest)
    if f.ndim != 1 or f.shape[0] != sym.nnz:
        raise ValueError("validate_spanning_forest: %d marks for the %d entries of the symmetric matrix" % (f.shape[0] if f.ndim == 1 else -1, sym.nnz))
    n = sym.num_rows
    f = f != 0
    indptr = sym.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = sym.adj_indices.astype(np.int64)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    mirror = np.searchsorted(rows * n + cols, cols * n + rows)               # (the matrix has no diagonal: every entry has one)
    if np.any(f != f[mirror]):
        j = first(f != f[mirror])
        raise ValueError("validate_spanning_forest: entry %d (%d, %d) is marked %d, its mirror entry %d (rule 1)"
                         % (j, rows[j], cols[j], f[j], f[mirror[j]]))
    edges = int(np.count_nonzero(f & (cols > rows)))
    want = _components_of(sym.adj_indptr, sym.adj_indices, None, n)
    kept = np.flatnonzero(f)
    kept_indptr = np.concatenate([[0], np.cumsum(np.bincount(rows[kept], minlength=n))])
    got = _components_of(kept_indptr, cols[kept], None, n)
    classes, components = int(np.count_nonzero(got == np.arange(n))), int(np.count_nonzero(want == np.arange(n)))
    if edges + classes != n:
        raise ValueError("validate_spanning_forest: the %d marked edges join the %d vertices into %d classes: %d of them close a cycle (rule 2)"
                         % (edges, n, classes, edges + classes - n))
    if np.any(got != want):
        v = first(got != want)
        raise ValueError("validate_spanning_forest: vertex %d is joined to %d by the graph's edges and not by the marked ones: the forest "
                         "has %d edges and the graph %d components on %d vertices, an edge is missing (rule 2)" % (v, want[v], edges, components, n))
    own = _kruskal_of(sym)
    if np.any(own != f):
        j = first(own != f)
        raise ValueError("validate_spanning_forest: entry %d (%d, %d) of weight %r is %s, and the minimum spanning forest under the order "
                         "(key(w), lo, hi) %s it (rule 3)" % (j, rows[j], cols[j], float(sym.adj_data[j]), "marked" if f[j] else "not marked",
                                                              "leaves out" if f[j] else "holds"))
    return edges


MATCH_FREE = np.uint32(0xffffffff)      # gl_match: mate[v] of a vertex that stays free


def _matching_graph_of(csr, weighted=True, drop_nonpositive=False):
    """the undirected weighted graph Matching reads out of `csr` -> (symmetric CSRMatrix, degrees): io.symmetrize_weighted with
    keep="largest" (an edge stored more than once gets its largest value); drop_nonpositive removes the edges of weight <= 0"""
    sym, deg = io.symmetrize_weighted(csr, weighted, keep="largest")
    if drop_nonpositive and sym.nnz and np.any(sym.adj_data <= 0):
        n = sym.num_rows
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
        keep = sym.adj_data > 0
        deg = np.bincount(rows[keep], minlength=n).astype(np.uint32)
        indptr = np.concatenate([[0], np.cumsum(deg, dtype=np.int64)]).astype(np.uint32)
        sym = io.CSRMatrix(n, n, sym.adj_data[keep], sym.adj_indices[keep], indptr)
    return sym, deg


def _greedy_matching_of(sym):
    """The greedy matching of a symmetric CSRMatrix with weights in adj_data, the edges taken in gl_match's order (~key(w), lo, hi)
    -- heaviest first, among equal weights the smallest (lo, hi) first: the entries above the diagonal sorted by (~key, entry
    number), one pass on the host that keeps an edge iff both its ends are free (kept apart from the device's pointer rounds:
    validate_matching checks one with the other) -> uint32[n] mates, MATCH_FREE for a free vertex."""
    n = sym.num_rows
    indptr = sym.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = sym.adj_indices.astype(np.int64)
    up = np.flatnonzero(cols > rows)
    up = up[np.argsort(~_edge_keys(sym.adj_data[up]), kind="stable")]       # (stable: ties stay in entry order = (lo, hi) order)
    mate = [-1] * n
    for u, v in zip(rows[up].tolist(), cols[up].tolist()):
        if mate[u] < 0 and mate[v] < 0:
            mate[u], mate[v] = v, u
    return (np.asarray(mate, dtype=np.int64) & 0xffffffff).astype(np.uint32)


def validate_matching(csr, mate, weighted=True, drop_nonpositive=False):
    """Host-side check (numpy) that `mate` is THE greedy matching of the undirected weighted graph of `csr` -- as Matching reads
    it: io.symmetrize_weighted(csr, weighted, keep="largest"), without the edges of weight <= 0 with drop_nonpositive -- one word
    per vertex of that symmetric matrix, as Matching.run() returns them.  Raises ValueError naming the first offending vertex
    or edge and the rule; returns the number of matched edges.  The rules:
      1. mate is an involution without fixed points: mate[v] is MATCH_FREE or a vertex u != v with mate[u] == v;
      2. every pair {v, mate[v]} is a stored edge;
      3. the matching is maximal: no edge has two free ends;
      4. it is the unique greedy one under the order (~key(w), lo, hi): it equals, vertex for vertex, what a host pass taking the
         edges in that order returns."""
    sym, _ = _matching_graph_of(csr, weighted, drop_nonpositive)
    m = np.asarray(mate)
    n = sym.num_rows
    if m.ndim != 1 or m.shape[0] != n:
        raise ValueError("validate_matching: %d mates for the %d vertices of the symmetric matrix" % (m.shape[0] if m.ndim == 1 else -1, n))
    m = m.astype(np.int64)
    free = m == int(MATCH_FREE)
    v = np.arange(n, dtype=np.int64)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    back = np.where(free, v, m[np.where(free | (m >= n), 0, m)])
    bad = ~free & ((m >= n) | (m == v) | (back != v))
    if np.any(bad):
        x = first(bad)
        if m[x] >= n:
            what = "is no vertex"
        elif m[x] == x:
            what = "is itself"
        else:
            what = "is free" if back[x] == int(MATCH_FREE) else "is matched to %d" % back[x]
        raise ValueError("validate_matching: vertex %d is matched to %d, which %s (rule 1)" % (x, m[x], what))
    rows = np.repeat(v, np.diff(sym.adj_indptr.astype(np.int64)))
    cols = sym.adj_indices.astype(np.int64)
    stored = np.zeros(n, dtype=bool)
    stored[rows[m[rows] == cols]] = True
    if np.any(~free & ~stored):
        x = first(~free & ~stored)
        raise ValueError("validate_matching: vertex %d is matched to %d, and (%d, %d) is no edge of the graph (rule 2)" % (x, m[x], x, m[x]))
    open_ = free[rows] & free[cols]
    if np.any(open_):
        j = first(open_)
        raise ValueError("validate_matching: both ends of edge (%d, %d) of weight %r are free: the matching is not maximal (rule 3)"
                         % (rows[j], cols[j], float(sym.adj_data[j])))
    own = _greedy_matching_of(sym).astype(np.int64)
    if np.any(own != m):
        x = first(own != m)

        def name(u):
            return "free" if u == int(MATCH_FREE) else "matched to %d" % u
        raise ValueError("validate_matching: vertex %d is %s, and in the greedy matching under the order (~key(w), lo, hi) it is %s (rule 4)"
                         % (x, name(m[x]), name(own[x])))
    return int(np.count_nonzero(~free)) // 2


LPA_NO_LABEL = 0xffffffff      # gl_lpa: the word no initial label may be (the empty key of the label tables)


def _lpa_row_modes(sym, labels):
    """for every vertex of the symmetric simple graph `sym` under `labels` -> (best, cur) as int64[n]: the largest number of
    neighbours that share one label, and the number of neighbours carrying the vertex's own label (0, 0 for an isolated vertex)"""
    n = sym.num_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
    cols = sym.adj_indices.astype(np.int64)
    off = rows != cols
    rows, cols = rows[off], cols[off]
    _, ident = np.unique(labels, return_inverse=True)                    # labels as numbers below n
    ident = ident.astype(np.int64)
    key, count = np.unique(rows * n + ident[cols], return_counts=True)
    best = np.zeros(n, dtype=np.int64)
    np.maximum.at(best, key // n, count)
    own = np.arange(n, dtype=np.int64) * n + ident
    at = np.minimum(np.searchsorted(key, own), max(key.shape[0] - 1, 0))
    cur = np.where(key[at] == own, count[at], 0) if key.shape[0] else np.zeros(n, dtype=np.int64)
    return best, cur


def _lpa_color_loop(sym, colors, initial, max_sweeps):
    """gl_lpa's colour-class schedule restated on the host -> (labels, sweeps, changes, evaluations, converged): the vertices
    with a neighbour in (colour, vertex) order, one after the other in place; a vertex is evaluated in sweep 1, and later iff a
    neighbour changed since its previous evaluation.  One np.unique per evaluation (kept apart from the device's tables and
    from the suite's dictionary loop: validate_communities checks one with the other)."""
    n = sym.num_rows
    indptr = sym.adj_indptr.astype(np.int64)
    cols = sym.adj_indices.astype(np.int64)
    label = np.asarray(initial, dtype=np.int64).copy()
    hood = [cols[indptr[v]:indptr[v + 1]] for v in range(n)]
    hood = [h[h != v] for v, h in enumerate(hood)]
    linked = np.array([h.shape[0] > 0 for h in hood], dtype=bool)
    order = [int(v) for v in np.lexsort((np.arange(n), np.asarray(colors, dtype=np.int64))) if linked[v]]
    active = linked.copy()
    sweeps = changes = evaluations = converged = 0
    while sweeps < max_sweeps and not converged:
        sweeps += 1
        changed = 0
        for v in order:
            if not active[v]:
                continue
            active[v] = False
            evaluations += 1
            seen, count = np.unique(label[hood[v]], return_counts=True)
            top = int(count.max())
            at = np.searchsorted(seen, label[v])
            cur = int(count[at]) if at < seen.shape[0] and seen[at] == label[v] else 0
            if top > cur:
                label[v] = seen[int(np.argmax(count))]                  # (the first maximum: seen ascends, so the smallest label)
                active[hood[v]] = True
                changed += 1
        changes += changed
        converged = int(changed == 0)
    return label.astype(np.uint32), sweeps, changes, evaluations, converged


def validate_communities(csr, labels, colors=None, initial=None, max_sweeps=None):
    """Host-side check (numpy) that `labels` is what label propagation leaves on the undirected simple graph of `csr` -- as
    LabelPropagation reads it: io.symmetrize_simple -- one word per vertex of that symmetric matrix, as LabelPropagation.run()
    returns them.  `initial`: the labels the run started from (default: every vertex's own number); `colors`: the colouring it
    swept by (None: the synchronous schedule, or unknown); `max_sweeps`: the cap it ran under (None: the labels are claimed to
    be a fixed point).  Raises ValueError naming the first offending vertex and the rule; returns the number of distinct labels.
      1. every label is one of the initial labels;
      2. a vertex without a neighbour keeps its initial label;
      3. if the run converged -- max_sweeps is None, or the host loop of rule 4 converged within it -- the labels are a fixed
         point: every vertex with a neighbour carries a label that a maximum number of its neighbours carry;
      4. with `colors`, the labels equal, vertex for vertex, what the host loop over the vertices in (colour, vertex) order
         leaves after at most max_sweeps sweeps (None: run to the fixed point)."""
    sym, deg = io.symmetrize_simple(csr)
    n = sym.num_rows
    got = np.asarray(labels)
    if got.ndim != 1 or got.shape[0] != n:
        raise ValueError("validate_communities: %d labels for the %d vertices of the symmetric matrix" % (got.shape[0] if got.ndim == 1 else -1, n))
    got = got.astype(np.int64)
    start = np.arange(n, dtype=np.int64)
    if initial is not None:
        given = np.asarray(initial).astype(np.int64)
        if given.ndim != 1 or given.shape[0] > n:
            raise ValueError("validate_communities: %d initial labels for %d vertices" % (given.shape[0] if given.ndim == 1 else -1, n))
        start[:given.shape[0]] = given

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    alien = ~np.isin(got, start)
    if np.any(alien):
        x = first(alien)
        raise ValueError("validate_communities: vertex %d carries the label %d, which no vertex started with (rule 1)" % (x, got[x]))
    moved = (deg == 0) & (got != start)
    if np.any(moved):
        x = first(moved)
        raise ValueError("validate_communities: vertex %d has no neighbour and carries %d, not its initial label %d (rule 2)" % (x, got[x], start[x]))
    converged = max_sweeps is None
    if colors is not None:
        col = np.asarray(colors).astype(np.int64)
        if col.ndim != 1 or col.shape[0] > n:
            raise ValueError("validate_communities: %d colours for %d vertices" % (col.shape[0] if col.ndim == 1 else -1, n))
        col = np.concatenate([col, np.zeros(n - col.shape[0], dtype=np.int64)])
        own, _, _, _, done = _lpa_color_loop(sym, col, start, (1 << 62) if max_sweeps is None else int(max_sweeps))
        converged = bool(done)
        if np.any(own.astype(np.int64) != got):
            x = first(own.astype(np.int64) != got)
            raise ValueError("validate_communities: vertex %d carries %d, and the loop in (colour, vertex) order leaves it %d (rule 4)"
                             % (x, got[x], own[x]))
    if converged:
        best, cur = _lpa_row_modes(sym, got)
        if np.any(cur < best):
            x = first(cur < best)
            raise ValueError("validate_communities: %d neighbours of vertex %d carry its label %d and %d carry another one: not a fixed "
                             "point (rule 3)" % (cur[x], x, got[x], best[x]))
    return int(np.unique(got).shape[0])


def _modularity_of(graph, degrees, labels):
    """-> float: Newman's modularity sum_c e_c / m - (d_c / 2 m)^2 of `labels` (one per vertex) on the symmetric simple graph
    `graph` with the degrees `degrees`, on the host in f64: e_c = edges inside community c, d_c = the degrees of its vertices,
    m = edges (0.0 for a graph without edges).  LabelPropagation.modularity and Louvain.modularity."""
    g = graph
    if g.nnz == 0:
        return 0.0
    _, ident = np.unique(labels, return_inverse=True)
    rows = np.repeat(np.arange(g.num_rows, dtype=np.int64), np.diff(g.adj_indptr.astype(np.int64)))
    inside = np.bincount(ident[rows][ident[rows] == ident[g.adj_indices.astype(np.int64)]], minlength=int(ident.max()) + 1)   # (twice e_c)
    degree = np.bincount(ident, weights=np.asarray(degrees).astype(np.float64), minlength=inside.shape[0])
    two_m = float(g.nnz)
    return float(np.sum(inside / two_m - (degree / two_m) ** 2))


def _louvain_entries(sym, weights):
    """-> (rows, cols, w) as int64 over the off-diagonal entries of `sym`; weights None: all 1"""
    n = sym.num_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
    cols = sym.adj_indices.astype(np.int64)
    w = np.ones(cols.shape[0], dtype=np.int64) if weights is None else np.asarray(weights).astype(np.int64)
    off = rows != cols
    return rows[off], cols[off], w[off]


def _louvain_move_loop(sym, weights, vertex_weights, colors, max_sweeps, min_gain):
    """gl_louvain_move restated on the host -> (labels, sweeps, moves, evaluations, stop reason, q_first, q_last): class by
    class, every vertex of a class decides from the labels and tot as they stand when the class begins, in numpy over the
    class's entries (one np.unique per class: kept apart from the device's tables and from the suite's dictionary loop;
    validate_louvain checks one with the other).  int64 throughout: two_m < 2^31 keeps every product below 2^62."""
    n = sym.num_rows
    rows, cols, w = _louvain_entries(sym, weights)
    if vertex_weights is None:
        k = np.zeros(n, dtype=np.int64)
        np.add.at(k, rows, w)
    else:
        k = np.asarray(vertex_weights).astype(np.int64)
    two_m = int(k.sum())
    if two_m >= 1 << 31:
        raise ValueError("_louvain_move_loop: two_m = %d >= 2^31" % two_m)
    label = np.arange(n, dtype=np.int64)
    tot = k.copy()
    inner = int(k.sum()) - int(w.sum())

    def q_of():
        return two_m * (inner + int(w[label[rows] == label[cols]].sum())) - int((tot * tot).sum())

    q_first = q_last = q_of()
    if rows.shape[0] == 0:
        return label.astype(np.uint32), 1, 0, 0, 1, 0, 0
    col = np.asarray(colors).astype(np.int64)
    by_class = np.argsort(col[rows], kind="stable")
    bounds = np.searchsorted(col[rows][by_class], np.arange(int(col.max()) + 2))
    linked = int(np.unique(rows).shape[0])
    sweeps = moves = evaluations = reason = 0
    while True:
        sweeps += 1
        moved = 0
        evaluations += linked
        for c in range(bounds.shape[0] - 1):
            e = by_class[bounds[c]:bounds[c + 1]]
            if e.shape[0] == 0:
                continue
            r, lab, ww = rows[e], label[cols[e]], w[e]
            key, inverse = np.unique(r * n + lab, return_inverse=True)
            kin = np.zeros(key.shape[0], dtype=np.int64)
            np.add.at(kin, inverse.reshape(-1), ww)
            kr, kl = key // n, key % n
            own = kl == label[kr]
            vs, at = np.unique(kr, return_inverse=True)                # the class's vertices only: cur of each, then per key
            at = at.reshape(-1)
            cur = -k[vs] * (tot[label[vs]] - k[vs])
            cur[at[own]] += two_m * kin[own]
            kr, kl, score, cur = kr[~own], kl[~own], (two_m * kin - k[kr] * tot[kl])[~own], cur[at][~own]
            first = np.lexsort((kl, -score, kr))                       # per vertex: the largest score, then the smallest label
            kr, kl, score, cur = kr[first], kl[first], score[first], cur[first]
            head = np.ones(kr.shape[0], dtype=bool)
            head[1:] = kr[1:] != kr[:-1]
            go = head & (score > cur)
            v, to = kr[go], kl[go]
            np.subtract.at(tot, label[v], k[v])
            np.add.at(tot, to, k[v])
            label[v] = to
            moved += int(v.shape[0])
        moves += moved
        q_old, q_last = q_last, q_of()
        if moved == 0:
            reason = 1
            break
        if q_last - q_old <= min_gain:
            reason = 2
            break
        if sweeps >= max_sweeps:
            break
    return label.astype(np.uint32), sweeps, moves, evaluations, reason, q_first, q_last


def _greedy_coloring_of(sym, prio):
    """-> uint32[n]: the first-fit greedy colouring in gl_color's order (larger priority first, ties to the smaller vertex
    number; prio None: ascending vertex order), the sequential loop"""
    n = sym.num_rows
    indptr = sym.adj_indptr.astype(np.int64).tolist()
    cols = sym.adj_indices.astype(np.int64).tolist()
    order = range(n) if prio is None else np.lexsort((np.arange(n), -np.asarray(prio).astype(np.int64))).tolist()
    color = [-1] * n
    for v in order:
        used = {color[u] for u in cols[indptr[v]:indptr[v + 1]] if u != v}
        c = 0
        while c in used:
            c += 1
        color[v] = c
    return np.asarray(color, dtype=np.uint32)


def _smallest_member_labels(community_of, n):
    """-> uint32[n]: every vertex labelled with the smallest vertex of its community"""
    community_of = np.asarray(community_of).astype(np.int64)
    smallest = np.full(int(community_of.max()) + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, community_of, np.arange(n, dtype=np.int64))
    return smallest[community_of].astype(np.uint32)


def _louvain_levels(sym, degrees, move, color, tol, max_sweeps, max_levels):
    """Louvain's level loop, shared by the driver (move and color run on the device) and the host model (they run on the
    host) -> a dict of the results.  move(level, graph, weights, k, colors, min_gain) -> (labels, sweeps, moves, evaluations,
    launches-or-0, reason, q_first, q_last); color(level, graph, degrees) -> (colors, num_colors).  Level 0 is `sym` with every
    weight 1 and k = degrees; a level is ACCEPTED iff it moved something and its q_last is strictly above the last accepted Q
    (at the start: the singletons' Q); otherwise it is discarded and the run ends, as it does when a level merges nothing or
    max_levels is reached."""
    n = sym.num_rows
    graph, weights, k = sym, None, np.asarray(degrees).astype(np.uint32)
    community_of = np.arange(n, dtype=np.int64)
    out = {"sizes": [], "colors": [], "sweeps": [], "moves": [], "q": [], "dendrogram": [], "colorings": [], "launches": 0, "levels": 0}
    accepted = None
    for level in range(max_levels):
        deg = np.diff(graph.adj_indptr.astype(np.int64)).astype(np.uint32)
        colors, num_colors = color(level, graph, deg)
        two_m = int(k.astype(np.int64).sum())
        min_gain = int(math.floor(tol * float(two_m * two_m)))
        labels, sweeps, moves, _, launches, _, q_first, q_last = move(level, graph, weights, k, colors, min_gain)
        out["sizes"].append(int(graph.num_rows))
        out["colors"].append(int(num_colors))
        out["colorings"].append(colors)
        out["sweeps"].append(int(sweeps))
        out["moves"].append(int(moves))
        out["q"].append((int(q_first), int(q_last)))
        out["launches"] += int(launches)
        if accepted is None:
            accepted = int(q_first)
        if moves == 0 or int(q_last) <= accepted:
            break
        accepted = int(q_last)
        smaller, weights, k, part = io.aggregate_communities(graph, weights, k, labels[:graph.num_rows])
        community_of = part.astype(np.int64)[community_of]
        out["dendrogram"].append(community_of.astype(np.uint32))
        out["levels"] += 1
        if smaller.num_rows == graph.num_rows:
            break
        graph = smaller
    out["labels"] = _smallest_member_labels(community_of, n)
    return out


def _louvain_host(sym, degrees, tol, max_sweeps, max_levels, order, seed, colorings=None):
    """the level loop with the host move loop and the host greedy colouring (colorings: one array per level overrides it)"""
    def color(level, graph, deg):
        if colorings is not None and level < len(colorings):
            c = np.asarray(colorings[level]).astype(np.uint32)[:graph.num_rows]
        else:
            if order == "smallest_last":
                raise ValueError("_louvain_host: the peeling order of \"smallest_last\" is not unique: pass the colourings the run used")
            c = _greedy_coloring_of(graph, io.coloring_priorities(deg, order, seed))
        return c, (int(c.max()) + 1 if c.shape[0] else 0)

    def move(level, graph, weights, k, colors, min_gain):
        lab, sweeps, moves, evals, reason, q0, q1 = _louvain_move_loop(graph, weights, k, colors, max_sweeps, min_gain)
        return lab, sweeps, moves, evals, 0, reason, q0, q1
    return _louvain_levels(sym, degrees, move, color, tol, max_sweeps, max_levels)


def validate_louvain(csr, labels, tol=1e-7, max_sweeps=100, max_levels=32, order="largest_first", seed=0, colorings=None):
    """Host-side check (numpy) that `labels` is what Louvain.run(tol, max_sweeps, max_levels, order, seed) leaves on the
    undirected simple graph of `csr` -- as Louvain reads it: io.symmetrize_simple -- one word per vertex of that symmetric
    matrix.  `colorings` (Louvain.level_colorings_: one colouring per level) replaces the host's greedy colourings; the
    "smallest_last" order needs them, because gl_kcore's peeling order is not unique.  Raises ValueError naming the first
    offending vertex and the rule; returns the number of communities.
      1. every vertex carries the smallest vertex number of its community: labels[v] <= v and labels[labels[v]] == labels[v];
      2. a vertex without a neighbour carries its own number;
      3. the labels equal, vertex for vertex, what the host model of the level loop leaves (_louvain_host)."""
    sym, deg = io.symmetrize_simple(csr)
    n = sym.num_rows
    got = np.asarray(labels)
    if got.ndim != 1 or got.shape[0] != n:
        raise ValueError("validate_louvain: %d labels for the %d vertices of the symmetric matrix" % (got.shape[0] if got.ndim == 1 else -1, n))
    got = got.astype(np.int64)
    own = np.arange(n, dtype=np.int64)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    bad = (got > own) | (got < 0)
    bad |= got[np.minimum(np.maximum(got, 0), n - 1)] != got
    if np.any(bad):
        x = first(bad)
        raise ValueError("validate_louvain: vertex %d carries %d, which is not the smallest vertex of a community (rule 1)" % (x, got[x]))
    alone = (deg == 0) & (got != own)
    if np.any(alone):
        x = first(alone)
        raise ValueError("validate_louvain: vertex %d has no neighbour and carries %d, not its own number (rule 2)" % (x, got[x]))
    want = _louvain_host(sym, deg, tol, max_sweeps, max_levels, order, seed, colorings)["labels"].astype(np.int64)
    if np.any(want != got):
        x = first(want != got)
        raise ValueError("validate_louvain: vertex %d carries %d, and the host model of the level loop leaves it %d (rule 3)" % (x, got[x], want[x]))
    return int(np.unique(got).shape[0])


def _pattern_as_scipy(csr, n):
    """the entries of a CSRMatrix as an n x n scipy matrix of f64 ones (the matrix may have fewer rows and columns)"""
    import scipy.sparse as sp
    ip = np.asarray(csr.adj_indptr).astype(np.int64)[:csr.num_rows + 1]
    ip = np.concatenate([ip, np.full(n - csr.num_rows, ip[-1], dtype=np.int64)])
    nnz = int(ip[-1])
    return sp.csr_matrix((np.ones(nnz, dtype=np.float64), np.asarray(csr.adj_indices[:nnz]).astype(np.int64), ip), shape=(n, n))


def _bfs_levels_of(A_out, sources, n):
    """The drivers' level array (float32[n]: 1 on every source, it + 1 on a vertex reached in iteration it, 0 unreached) of a
    complete search on the host; A_out is the scipy matrix whose row u holds the out-neighbours of u."""
    level = np.zeros(n, dtype=np.float32)
    frontier = np.unique(np.asarray(sources, dtype=np.int64))
    level[frontier] = 1.0
    it = 1
    ip, idx = A_out.indptr, A_out.indices
    while frontier.size:
        starts, lens = ip[frontier], ip[frontier + 1] - ip[frontier]
        total = int(lens.sum())
        if not total:
            break
        at = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
        nxt = np.unique(idx[at])
        frontier = nxt[level[nxt] == 0]
        it += 1
        level[frontier] = float(it)
    return level


def betweenness_by_levels(csr_in, csr_out, level):
    """gl_bc_accumulate's definition on the host, in f64, one scipy SpMV per level -> (sigma, delta), float64[n] each, n =
    len(level).  Row v of `csr_in` lists the vertices v is pulled from, row u of `csr_out` (None: the pattern is symmetric) the
    out-neighbours of u; `level` are the drivers' levels (1 on every source, 0 unreached), D their maximum:
      sigma[v] = 1 on level 1; the sum over u in row_in(v) with level[u] == level[v] - 1 of sigma[u] on level >= 2; 0 on level 0
      delta[u] = sigma[u] * the sum over v in row_out(u) with level[v] == level[u] + 1 and sigma[v] > 0 of (1 + delta[v]) / sigma[v]
    A vertex of level >= 2 without an in-neighbour one level up (not a BFS result) has sigma 0 and contributes nothing.  If a
    sigma is not finite, delta is all zero: the device does not run the backward sweep then."""
    lev = np.asarray(level).astype(np.int64)
    n = lev.shape[0]
    A_in = _pattern_as_scipy(csr_in, n)
    A_out = A_in if csr_out is None else _pattern_as_scipy(csr_out, n)
    D = int(lev.max()) if n else 0
    sigma = (lev == 1).astype(np.float64)
    delta = np.zeros(n, dtype=np.float64)
    # the vertices bucketed by level, as the device buckets them: a level's SpMV multiplies that level's rows only, by a
    # vector that holds the neighbouring level's values and zeros elsewhere
    order = np.argsort(lev, kind="stable")
    off = np.searchsorted(lev[order], np.arange(D + 3))
    rows = [order[off[L]:off[L + 1]] for L in range(D + 2)]
    x = np.zeros(n, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for L in range(2, D + 1):
            x[rows[L - 1]] = sigma[rows[L - 1]]
            if rows[L].size:
                sigma[rows[L]] = A_in[rows[L]] @ x
            x[rows[L - 1]] = 0.0
        if not np.all(np.isfinite(sigma)):
            return sigma, delta
        coef = np.zeros(n, dtype=np.float64)
        for L in range(D, 0, -1):
            r = rows[L]
            if L < D and r.size:
                x[rows[L + 1]] = coef[rows[L + 1]]
                delta[r] = sigma[r] * (A_out[r] @ x)
                x[rows[L + 1]] = 0.0
            live = r[sigma[r] > 0]
            coef[live] = (1.0 + delta[live]) / sigma[live]
    return sigma, delta


def _bc_scale(n, k, normalized, directed):
    """networkx's _rescale for endpoints=False (betweenness.py, 3.4.2) as one factor: n vertices, k sources.  Where networkx
    does not rescale at all (directed and not normalised, or normalised with n <= 2) it does not apply n / k either."""
    if normalized:
        scale = 1.0 / ((n - 1) * (n - 2)) if n > 2 else None
    else:
        scale = None if directed else 0.5
    if scale is None:
        return 1.0
    return scale * n / k if k < n else scale


def _bc_patterns(csr, directed):
    """-> (csr_in, csr_out or None, directed): what BetweennessCentrality.load_and_format_matrix loads for `directed`"""
    cin, cout, symmetric = io.simple_pattern(csr)
    if directed is None:
        directed = not symmetric
    if not directed and not symmetric:
        cin, cout = io.symmetrize_simple(csr)[0], None
    elif directed and symmetric:
        cout = cin.copy()
    return cin, cout, bool(directed)


def validate_betweenness(csr, bc, sources=None, normalized=False, directed=None):
    """Host-side check (numpy / scipy) that `bc` is the betweenness centrality of the simple graph of `csr` -- an edge u -> v
    iff u != v and a stored non-zero entry A[v, u] exists; directed=None reads it as undirected iff that pattern is
    symmetric, False takes every edge in both directions -- summed over `sources` (None: all csr.num_rows vertices) and scaled
    as networkx.betweenness_centrality(endpoints=False) scales: recomputed from host BFS levels (betweenness_by_levels).  Raises
    ValueError naming the first offender; returns the largest relative error.  The bound is derived, not measured: every term
    is >= 0, so a value's relative error is at most the roundings on its longest chain times 2^-53:
    4 (D (longest row + 4) + sources) 2^-53, D the deepest search -- device and host round independently.  Zeros must be zeros.
    `bc` may be longer than the matrix (the drivers pad it): the extra vertices must hold 0."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    got = np.asarray(bc, dtype=np.float64)
    n = got.shape[0] if got.ndim == 1 else -1
    if n < max(nr, nc):
        raise ValueError("validate_betweenness: %d values for a %d x %d matrix" % (n, nr, nc))
    cin, cout, directed = _bc_patterns(csr, directed)
    A_in = _pattern_as_scipy(cin, n)
    A_out = A_in if cout is None else _pattern_as_scipy(cout, n)
    src = list(range(nr)) if sources is None else [int(s) for s in sources]
    if any(s < 0 or s >= nr for s in src):
        raise ValueError("validate_betweenness: a source outside 0 .. %d" % (nr - 1))
    scale = _bc_scale(nr, len(src), normalized, directed)
    want = np.zeros(n, dtype=np.float64)
    depth = 1
    for s in src:
        level = _bfs_levels_of(A_out, [s], n)
        sigma, delta = betweenness_by_levels(cin, cout, level)
        if not np.all(np.isfinite(sigma)):
            continue                                         # (the drivers skip such a source and say so)
        want += np.where(level >= 2, scale * delta, 0.0)
        depth = max(depth, int(level.max()))
    longest = max(int(np.diff(A_in.indptr).max()), int(np.diff(A_out.indptr).max())) if n else 0
    bound = 4.0 * (depth * (longest + 4) + len(src)) * 2.0 ** -53
    if np.any(got[nr:] != 0):
        v = nr + int(np.flatnonzero(got[nr:] != 0)[0])
        raise ValueError("validate_betweenness: padding vertex %d is given %.17g" % (v, got[v]))
    if not np.array_equal(got == 0, want == 0):
        v = int(np.flatnonzero((got == 0) != (want == 0))[0])
        raise ValueError("validate_betweenness: vertex %d is given %.17g, its betweenness is %.17g" % (v, got[v], want[v]))
    miss = ~(np.abs(got - want) <= bound * want)
    if np.any(miss):
        v = int(np.flatnonzero(miss)[0])
        raise ValueError("validate_betweenness: vertex %d is given %.17g, its betweenness is %.17g (relative bound %.3g)"
                         % (v, got[v], want[v], bound))
    live = want > 0
    return float(np.max(np.abs(got[live] - want[live]) / want[live])) if np.any(live) else 0.0


def _edges_of_pattern(csr, n):
    """-> (src, dst), int64 each: the edges u -> v of the simple directed graph of `csr` among the first n vertices -- u != v, a
    stored non-zero entry A[v, u]; duplicates stay (they change no reachability)"""
    ip = np.asarray(csr.adj_indptr).astype(np.int64)[:csr.num_rows + 1]
    nnz = int(ip[-1])
    dst = np.repeat(np.arange(csr.num_rows, dtype=np.int64), np.diff(ip))
    src = np.asarray(csr.adj_indices[:nnz]).astype(np.int64)
    keep = (np.asarray(csr.adj_data[:nnz]) != 0) & (src != dst) & (src < n) & (dst < n)
    return src[keep], dst[keep]


def _reach_inside(src, dst, start, n):
    """-> bool[n]: the vertices reached from the vertices `start` (bool[n]) along the edges src[i] -> dst[i], whole sweeps in numpy"""
    seen = start.copy()
    while True:
        step = np.zeros(n, dtype=bool)
        step[dst[seen[src]]] = True
        step &= ~seen
        if not step.any():
            return seen
        seen |= step


def validate_strong_components(csr, labels):
    """Host-side check (numpy) that `labels` are the strongly connected components of the simple directed graph of `csr` -- an
    edge u -> v iff u != v and a stored non-zero entry A[v, u] exists -- each vertex labelled with the SMALLEST vertex of its
    component.  Raises ValueError naming the first offender and the rule; returns the number of components among the vertices
    `labels` covers.  The rules:
      1. labels[labels[v]] == labels[v] and labels[v] <= v;
      2. every class is strongly connected: inside the class, every member is reached from its label and reaches it;
      3. the classes are maximal: the graph between the classes (the condensation) has no cycle.
    `labels` may be longer than the matrix (the drivers pad it): the extra vertices have empty rows."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    lab = np.asarray(labels).astype(np.int64)
    n = lab.shape[0]
    if lab.ndim != 1 or n < max(nr, nc):
        raise ValueError("validate_strong_components: %d labels for a %d x %d matrix" % (n, nr, nc))

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    v = np.arange(n, dtype=np.int64)
    if np.any((lab < 0) | (lab > v)):
        k = first((lab < 0) | (lab > v))
        raise ValueError("validate_strong_components: vertex %d has label %d, which is above it (rule 1)" % (k, lab[k]))
    if np.any(lab[lab] != lab):
        k = first(lab[lab] != lab)
        raise ValueError("validate_strong_components: vertex %d has label %d, whose own label is %d (rule 1)" % (k, lab[k], lab[lab[k]]))
    src, dst = _edges_of_pattern(csr, n)
    inside = lab[src] == lab[dst]
    roots = lab == v
    forward = _reach_inside(src[inside], dst[inside], roots, n)
    if not forward.all():
        k = first(~forward)
        raise ValueError("validate_strong_components: vertex %d is not reached from its label %d inside its class (rule 2)" % (k, lab[k]))
    backward = _reach_inside(dst[inside], src[inside], roots, n)
    if not backward.all():
        k = first(~backward)
        raise ValueError("validate_strong_components: vertex %d does not reach its label %d inside its class (rule 2)" % (k, lab[k]))
    # Kahn's peeling of the condensation, a whole layer of classes at a time: what cannot be peeled lies on a cycle of classes
    a, b = lab[src[~inside]], lab[dst[~inside]]
    left = roots.copy()
    while a.size:
        fed = np.zeros(n, dtype=bool)
        fed[b] = True
        peel = left & ~fed
        if not peel.any():
            k = first(left & fed)
            raise ValueError("validate_strong_components: the class of label %d lies on a cycle of classes or behind one, so the classes "
                             "on that cycle are no whole components (rule 3)" % k)
        left &= ~peel
        keep = ~peel[a]
        a, b = a[keep], b[keep]
    return int(np.count_nonzero(roots))


class HipBackend:
    """Allocation / transfer hooks of the drivers.  The CPU tests substitute a stand-in with the
    same methods to exercise the distributed control flow over gloo."""
    SpMVModule = M.SpMVModule
    SpMSpVModule = M.SpMSpVModule
    eWiseAddModule = M.eWiseAddModule
    AssignVectorDenseModule = M.AssignVectorDenseModule
    AssignVectorSparseModule = M.AssignVectorSparseModule

    def __init__(self, device=0, use_torch=False):
        self.device = device
        self.use_torch = use_torch

    def init(self):
        capi.init(self.device)
        if self.use_torch:
            import torch
            torch.cuda.set_device(self.device)
            capi.set_stream(torch.cuda.current_stream().cuda_stream)

    def alloc(self, count, dtype):
        """Device array of `count` elements; dtype is np.float32 or capi.IDX_VAL.  In torch mode the
        buffer carries `.tensor` (float32, or int64 with one element per (index,val) pair)."""
        itemsize = np.dtype(dtype).itemsize
        if self.use_torch:
            import torch
            t = torch.zeros(count, dtype=torch.float32 if itemsize == 4 else torch.int64,
                            device="cuda:%d" % self.device)
            buf = capi.DeviceBuffer.from_torch(t)
            buf.tensor = t
            return buf
        buf = capi.DeviceBuffer(count * itemsize)
        buf.tensor = None
        return buf

    def view(self, buf, first, count, itemsize):
        v = capi.DeviceBuffer(count * itemsize, ptr=buf.ptr + first * itemsize, keepalive=buf)
        v.tensor = None
        return v

    def upload(self, buf, arr):
        buf.write(np.ascontiguousarray(arr))

    def download(self, buf, dtype, count):
        return buf.read(dtype, count)

    def download_result(self, buf, count):
        """Final float32 read-back of a driver: a fresh host array per call, like the by-value return
        of the reference's send_*_device_to_host.  (A page-locked destination -- capi.pinned_empty +
        read(out=) -- halves the copy time but must be reused across calls to pay off; measured: pinning
        12 MB per call costs more than it saves.)"""
        return buf.read(np.float32, count)

    def copy(self, dst, src, nbytes):
        capi.copy_d2d(dst, src, nbytes)

    def fill(self, buf, value, count):
        capi.fill_f32(buf, value, count)

    def sparse_to_dense(self, sparse, dense, rng, zero, max_entries):
        capi.sparse_to_dense(sparse, dense, rng, zero, max_entries)

    def sync(self):
        capi.sync()


def _mirror_entries(indptr, indices, n):
    """-> (rows, cols, mirror), int64 each: for every entry j = (v, u) of a symmetric matrix with ascending rows the number of the
    entry (u, v)"""
    ip = np.asarray(indptr).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip[:n + 1]))
    cols = np.asarray(indices[:ip[n]]).astype(np.int64)
    return rows, cols, np.searchsorted(rows * n + cols, cols * n + rows)


def _blocks_of(indptr, indices, n):
    """The biconnected components of a symmetric simple graph with ascending rows, by Hopcroft and Tarjan's depth-first search
    with a stack of edges (iterative, plain python; kept apart from the device's Tarjan-Vishkin: validate_biconnected checks one
    with the other) -> int64[nnz]: for every entry the smallest entry number of its block, -1 for an entry (v, v)."""
    ip = [int(x) for x in np.asarray(indptr).astype(np.int64)[:n + 1]]
    rows, cols, mirror = _mirror_entries(indptr, indices, n)
    cols_l, mirror_l = cols.tolist(), mirror.tolist()
    label = np.full(cols.shape[0], -1, dtype=np.int64)
    disc, low, via, nxt = [-1] * n, [0] * n, [-1] * n, ip[:n]
    clock, edges = 0, []
    for s in range(n):
        if disc[s] != -1 or ip[s] == ip[s + 1]:
            continue
        disc[s] = low[s] = clock
        clock += 1
        path = [s]
        while path:
            v = path[-1]
            if nxt[v] < ip[v + 1]:
                j = nxt[v]
                nxt[v] += 1
                u = cols_l[j]
                if u == v or (via[v] >= 0 and j == mirror_l[via[v]]):
                    continue
                if disc[u] == -1:
                    via[u] = j
                    disc[u] = low[u] = clock
                    clock += 1
                    edges.append(j)
                    path.append(u)
                elif disc[u] < disc[v]:
                    edges.append(j)
                    low[v] = min(low[v], disc[u])
            else:
                path.pop()
                if path:
                    p = path[-1]
                    low[p] = min(low[p], low[v])
                    if low[v] >= disc[p]:
                        cut = len(edges) - 1
                        while edges[cut] != via[v]:
                            cut -= 1
                        members = np.array(edges[cut:], dtype=np.int64)
                        del edges[cut:]
                        both = np.concatenate([members, mirror[members]])
                        label[both] = both.min()
    return label


def validate_biconnected(csr, block, vertex_blocks=None, edge_component=None):
    """Host-side check that `block` are the biconnected components of the undirected simple graph of `csr` -- an edge {u, v} iff u
    != v and a stored non-zero entry A[v, u] or A[u, v] exists -- one label per entry of io.symmetrize_simple(csr)[0], as
    BiconnectedComponents.run() returns them: the smallest entry number of the entry's block.  Raises ValueError naming the first
    offender and the rule; returns the number of blocks.  The rules:
      1. the two entries of an edge agree;
      2. a label is the smallest entry of its class: block[block[j]] == block[j] <= j;
      3. the classes equal those of a host Hopcroft-Tarjan search (_blocks_of);
      4. vertex_blocks[v] (optional) is the number of distinct labels in row v;
      5. edge_component (optional) passes validate_components on the graph without its bridges, the blocks of a single edge.
    `vertex_blocks` and `edge_component` may be longer than the matrix (the drivers pad it): the extra vertices are isolated."""
    sym, _ = io.symmetrize_simple(csr)
    b = np.asarray(block)
    if b.ndim != 1 or b.shape[0] != sym.nnz:
        raise ValueError("validate_biconnected: %d labels for the %d entries of the symmetric matrix" % (b.shape[0] if b.ndim == 1 else -1, sym.nnz))
    b = b.astype(np.int64)
    n, nnz = sym.num_rows, sym.nnz
    rows, cols, mirror = _mirror_entries(sym.adj_indptr, sym.adj_indices, n)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    if np.any(b != b[mirror]):
        j = first(b != b[mirror])
        raise ValueError("validate_biconnected: entry %d (%d, %d) is given block %d, its mirror entry %d block %d (rule 1)"
                         % (j, rows[j], cols[j], b[j], mirror[j], b[mirror[j]]))
    j_all = np.arange(nnz, dtype=np.int64)
    if np.any((b < 0) | (b > j_all)):
        j = first((b < 0) | (b > j_all))
        raise ValueError("validate_biconnected: entry %d has label %d, which is no entry at or below it (rule 2)" % (j, b[j]))
    if np.any(b[b] != b):
        j = first(b[b] != b)
        raise ValueError("validate_biconnected: entry %d has label %d, whose own label is %d (rule 2)" % (j, b[j], b[b[j]]))
    want = _blocks_of(sym.adj_indptr, sym.adj_indices, n)
    if np.any(want != b):
        j = first(want != b)
        raise ValueError("validate_biconnected: entry %d (%d, %d) is given block %d, a depth-first search finds its block's smallest entry to be %d "
                         "(rule 3)" % (j, rows[j], cols[j], b[j], want[j]))
    sizes = np.bincount(b, minlength=max(nnz, 1))
    if vertex_blocks is not None:
        vb = np.asarray(vertex_blocks).astype(np.int64)
        if vb.ndim != 1 or vb.shape[0] < n:
            raise ValueError("validate_biconnected: %d vertex_blocks for %d vertices" % (vb.shape[0] if vb.ndim == 1 else -1, n))
        pairs = np.unique(rows * max(nnz, 1) + b)
        distinct = np.bincount(pairs // max(nnz, 1), minlength=vb.shape[0])
        if np.any(distinct != vb):
            v = first(distinct != vb)
            raise ValueError("validate_biconnected: vertex %d lies in %d blocks, vertex_blocks says %d (rule 4)" % (v, distinct[v], vb[v]))
    if edge_component is not None:
        keep = sizes[b] != 2
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=n), out=indptr[1:])
        rest = io.CSRMatrix(n, n, np.ones(int(keep.sum()), dtype=np.float32), cols[keep].astype(np.uint32), indptr.astype(np.uint32))
        try:
            validate_components(rest, edge_component)
        except ValueError as e:
            raise ValueError("validate_biconnected: edge_component, on the graph without its bridges: %s (rule 5)" % e)
    return int(np.count_nonzero(sizes))


def _f32_keys(values):
    """-> uint64: the monotone map of the f32 bits (gl_msf.hip's key), which orders non-NaN floats as < does"""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(bits >> np.uint64(31) != 0, bits ^ np.uint64(0xFFFFFFFF), bits ^ np.uint64(0x80000000))


def _concat_ranges(start, length):
    """-> int64: start[0] .. start[0] + length[0] - 1, start[1] .. , ... in one array"""
    length = np.asarray(length, np.int64)
    total = int(length.sum())
    first = np.cumsum(length) - length
    return np.arange(total, dtype=np.int64) + np.repeat(np.asarray(start, np.int64) - first, length)


def _topological_of(n, src, dst, w=None):
    """Kahn's peeling, a whole level at a time in numpy, of the edges src[i] -> dst[i] (simple: no loops, no duplicates) with the
    f32 weights w[i] -> (level uint32[n], dist float32[n] or None, parent uint32[n] or None): gl_topo's definitions -- level =
    the edges of the longest path that ends in the vertex, 0xffffffff on a cycle or behind one; dist = the largest f32 dist[u] +
    w over the predecessors, +0 on a source, the bits 0x7fc00000 when unpeeled; parent = the smallest u that attains it."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    by_in = np.lexsort((src, dst))
    in_src = src[by_in]
    in_w = None if w is None else np.asarray(w, np.float32)[by_in]
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int64)
    by_out = np.argsort(src, kind="stable")
    out_dst = dst[by_out]
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    pending = np.diff(in_ptr)
    level = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    dist = parent = None
    if w is not None:
        dist = np.full(n, 0x7FC00000, dtype=np.uint32).view(np.float32)
        parent = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    front = np.flatnonzero(pending == 0)
    lvl = 0
    while front.size:
        level[front] = lvl
        if w is not None:
            dist[front] = 0.0
            fed = front[in_ptr[front + 1] > in_ptr[front]]
            if fed.size:
                lens = in_ptr[fed + 1] - in_ptr[fed]
                e = _concat_ranges(in_ptr[fed], lens)
                with np.errstate(over="ignore"):
                    cand = (dist[in_src[e]] + in_w[e]).astype(np.float32)
                word = (_f32_keys(cand) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - in_src[e].astype(np.uint64))
                best = np.maximum.reduceat(word, np.cumsum(lens) - lens)
                key = (best >> np.uint64(32)).astype(np.uint32)
                dist[fed] = np.where(key >> 31 != 0, key ^ np.uint32(0x80000000), ~key).view(np.float32)
                parent[fed] = (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.uint32)
        e = _concat_ranges(out_ptr[front], out_ptr[front + 1] - out_ptr[front])
        hit = np.bincount(out_dst[e], minlength=n)
        pending -= hit
        front = np.flatnonzero((hit > 0) & (pending == 0))
        lvl += 1
    return level, dist, parent


def validate_topological(csr, level, dist=None, parent=None, weighted=False):
    """Host-side check (numpy) that `level` -- and, with weighted=True, `dist` and `parent` -- are gl_topo's results on the directed
    graph of `csr` as io.directed_weighted(csr, weighted) reads it: an edge u -> v for a stored entry A[v, u], u != v (unweighted:
    a stored NON-ZERO entry).  Raises ValueError with the message of the first violation, naming the offender and the rule;
    returns the number of peeled vertices among those `level` covers.  The rules:
      1. every edge into a peeled vertex comes from a peeled vertex of a lower level;
      2. a peeled vertex without predecessors has level 0, every other one a predecessor exactly one level below;
      3. every unpeeled vertex (level 0xffffffff) has an unpeeled predecessor: it lies on a cycle or behind one;
      4. level, dist and parent equal the host loop's (Kahn's peeling a level at a time; dist and parent to the bit).
    The arrays may be longer than the matrix (the drivers pad it): the extra vertices are isolated."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    lev = np.asarray(level).astype(np.int64)
    n = lev.shape[0]
    if lev.ndim != 1 or n < max(nr, nc):
        raise ValueError("validate_topological: %d levels for a %d x %d matrix" % (n, nr, nc))
    if weighted and (dist is None or parent is None):
        raise ValueError("validate_topological: weighted=True needs dist and parent")

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    g = io.directed_weighted(csr, weighted)[0]
    dst = np.repeat(np.arange(g.num_rows, dtype=np.int64), np.diff(g.adj_indptr.astype(np.int64)))
    src = g.adj_indices.astype(np.int64)
    none = 0xFFFFFFFF
    peeled = lev != none
    into = peeled[dst]
    bad = into & (~peeled[src] | (lev[src] >= lev[dst]))
    if np.any(bad):
        k = first(bad)
        raise ValueError("validate_topological: the edge %d -> %d goes from level %s to level %d (rule 1)"
                         % (src[k], dst[k], "none" if lev[src[k]] == none else str(lev[src[k]]), lev[dst[k]]))
    has_pred = np.zeros(n, dtype=bool)
    has_pred[dst] = True
    below = np.zeros(n, dtype=bool)
    below[dst[into & (lev[src] + 1 == lev[dst])]] = True
    bad = peeled & ((~has_pred & (lev != 0)) | (has_pred & ~below))
    if np.any(bad):
        k = first(bad)
        raise ValueError("validate_topological: vertex %d has level %d and %s (rule 2)"
                         % (k, lev[k], "a predecessor one level below is missing" if has_pred[k] else "no predecessor"))
    waits = np.zeros(n, dtype=bool)
    waits[dst[~peeled[src]]] = True
    bad = ~peeled & ~waits
    if np.any(bad):
        k = first(bad)
        raise ValueError("validate_topological: vertex %d is not peeled and has no unpeeled predecessor (rule 3)" % k)
    w = g.adj_data if weighted else None
    want_level, want_dist, want_parent = _topological_of(n, src, dst, w)
    if not np.array_equal(want_level, lev.astype(np.uint32)):
        k = first(want_level != lev.astype(np.uint32))
        raise ValueError("validate_topological: vertex %d has level %d, the host loop gives %d (rule 4)" % (k, lev[k], want_level[k]))
    if weighted:
        got_dist = np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32)
        got_parent = np.asarray(parent).astype(np.uint32)
        if got_dist.shape != (n,) or got_parent.shape != (n,):
            raise ValueError("validate_topological: dist and parent must have %d words, as level" % n)
        if not np.array_equal(got_dist, want_dist.view(np.uint32)):
            k = first(got_dist != want_dist.view(np.uint32))
            raise ValueError("validate_topological: vertex %d has dist %r (bits 0x%08x), the host loop gives %r (rule 4)"
                             % (k, float(got_dist[k:k + 1].view(np.float32)[0]), got_dist[k], float(want_dist[k])))
        if not np.array_equal(got_parent, want_parent):
            k = first(got_parent != want_parent)
            raise ValueError("validate_topological: vertex %d has parent %d, the host loop gives %d (rule 4)" % (k, got_parent[k], want_parent[k]))
    return int(np.count_nonzero(peeled))


def _hops_of(A_out, s, n):
    """-> uint32[n]: the edges of a shortest path from s to every vertex on the host (0 on s, 0xffffffff unreached); A_out is the
    scipy matrix whose row u holds the out-neighbours of u."""
    hops = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    frontier = np.array([s], dtype=np.int64)
    hops[s] = 0
    ip, idx = A_out.indptr, A_out.indices
    d = 0
    while frontier.size:
        starts, lens = ip[frontier], ip[frontier + 1] - ip[frontier]
        total = int(lens.sum())
        if not total:
            break
        at = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
        nxt = np.unique(idx[at])
        frontier = nxt[hops[nxt] == 0xFFFFFFFF]
        d += 1
        hops[frontier] = d
    return hops


def _closeness_sums(hops_rows, batch=64):
    """gl_msbfs's three arrays from the sources' distance rows (uint32[k, n], 0xffffffff unreached), as a driver that deals the
    sources into batches of `batch` accumulates them -> (far uint64[n], reach uint32[n], harmonic float64[n]).  The harmonic
    sum is the device's ordered f64 loop: per batch the levels d ascending, c = the batch's sources at distance d, one division
    and one addition where c > 0."""
    hops_rows = np.asarray(hops_rows, dtype=np.uint32)
    k, n = hops_rows.shape
    far, reach, harmonic = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64)
    for b in range(0, k, batch):
        rows = hops_rows[b:b + batch]
        finite = rows[(rows != 0xFFFFFFFF) & (rows != 0)]
        for d in range(1, (int(finite.max()) if finite.size else 0) + 1):
            c = np.count_nonzero(rows == d, axis=0)
            hit = c > 0
            far[hit] += (c[hit] * d).astype(np.uint64)
            reach[hit] += c[hit].astype(np.uint32)
            harmonic[hit] = harmonic[hit] + c[hit].astype(np.float64) / np.float64(d)
    return far, reach, harmonic


def closeness_of(far, reach, n, wf_improved=True):
    """-> float64: the closeness centrality from gl_msbfs's integer arrays on a graph of n vertices, in f64 on the host: reach /
    far (0 where far == 0), times reach / (n - 1) with wf_improved (Wasserman and Faust's scaling for graphs that are not
    strongly connected) -- networkx.closeness_centrality's value when every vertex is a source."""
    far, reach = np.asarray(far).astype(np.float64), np.asarray(reach).astype(np.float64)
    live = far > 0
    out = np.zeros(far.shape[0], dtype=np.float64)
    out[live] = reach[live] / far[live]
    if wf_improved:
        out[live] = out[live] * (reach[live] / np.float64(n - 1)) if n > 1 else 0.0
    return out


def validate_closeness(csr, far, reach, harmonic=None, sources=None, directed=None, reverse=False, hops=None):
    """Host-side check (numpy / scipy) that `far`, `reach` -- and `harmonic` and `hops` when given -- are gl_msbfs's results on the
    simple graph of `csr`, as ClosenessCentrality reads it: an edge u -> v iff u != v and a stored non-zero entry A[v, u] exists;
    directed=None reads it as undirected iff that pattern is symmetric, False takes every edge in both directions.  `sources`
    (None: all csr.num_rows vertices) is the SEQUENCE the driver dealt into batches of 64; reverse=False measures the distances
    from the sources (what every vertex sums is its INCOMING distance), True the distances to them.  Everything is recomputed
    from one host BFS per source; the integers are compared exactly, `harmonic` as bits against the same ordered f64 loop,
    `hops` (uint32[len(sources), n]) word by word.  Raises ValueError with the first violation; returns the diameter found (the
    largest finite distance from a source).  The arrays may be longer than the matrix (the drivers pad it): the extra vertices
    are isolated and must hold 0."""
    nr, nc = int(csr.num_rows), int(csr.num_cols)
    got_far, got_reach = np.asarray(far), np.asarray(reach)
    n = got_far.shape[0] if got_far.ndim == 1 else -1
    if n < max(nr, nc) or got_reach.shape != (n,):
        raise ValueError("validate_closeness: %d and %d values for a %d x %d matrix" % (n, got_reach.shape[0] if got_reach.ndim == 1 else -1, nr, nc))
    src = list(range(nr)) if sources is None else [int(s) for s in sources]
    if any(s < 0 or s >= nr for s in src):
        raise ValueError("validate_closeness: a source outside 0 .. %d" % (nr - 1))
    if len(set(src)) != len(src):
        raise ValueError("validate_closeness: a source is given twice")
    cin, cout, directed = _bc_patterns(csr, directed)
    A_in = _pattern_as_scipy(cin, n)
    A_out = A_in.T.tocsr() if cout is None or not directed else _pattern_as_scipy(cout, n)      # row u: the out-neighbours of u
    walk = A_in if reverse else A_out
    walk.sort_indices()
    rows = np.empty((len(src), n), dtype=np.uint32)
    for j, s in enumerate(src):
        rows[j] = _hops_of(walk, s, n)
    want_far, want_reach, want_harmonic = _closeness_sums(rows)

    def first(bad):
        return int(np.flatnonzero(bad)[0])

    if hops is not None:
        got_hops = np.asarray(hops)
        if got_hops.shape != rows.shape:
            raise ValueError("validate_closeness: hops of shape %s, expected %s" % (got_hops.shape, rows.shape))
        bad = got_hops.astype(np.int64) != rows.astype(np.int64)
        if np.any(bad):
            j, v = (int(x[0]) for x in np.nonzero(bad))
            raise ValueError("validate_closeness: hops[%d, %d] is %d, vertex %d lies %d edges from source %d"
                             % (j, v, got_hops[j, v], v, rows[j, v], src[j]))
    bad = got_far.astype(np.uint64) != want_far
    if np.any(bad):
        v = first(bad)
        raise ValueError("validate_closeness: vertex %d has far %d, its distances sum to %d" % (v, got_far[v], want_far[v]))
    bad = got_reach.astype(np.int64) != want_reach.astype(np.int64)
    if np.any(bad):
        v = first(bad)
        raise ValueError("validate_closeness: vertex %d has reach %d, %d sources reach it" % (v, got_reach[v], want_reach[v]))
    if harmonic is not None:
        got_h = np.ascontiguousarray(harmonic, dtype=np.float64)
        if got_h.shape != (n,):
            raise ValueError("validate_closeness: harmonic must have %d values, as far" % n)
        bad = got_h.view(np.uint64) != want_harmonic.view(np.uint64)
        if np.any(bad):
            v = first(bad)
            raise ValueError("validate_closeness: vertex %d has harmonic %.17g (bits 0x%016x), the ordered loop gives %.17g"
                             % (v, got_h[v], got_h.view(np.uint64)[v], want_harmonic[v]))
    finite = rows[rows != 0xFFFFFFFF]
    return int(finite.max()) if finite.size else 0


SIMILARITY_MEASURES = ("common", "jaccard", "overlap", "sorensen", "cosine", "preferential_attachment", "adamic_adar",
                       "resource_allocation")


def similarity_shift(max_degree):
    """-> the fixed point of Similarity's weight tables: 62 - bit_length(max degree).  A weight is below 2^(shift + 1) (1 / ln 2
    < 2), a pair has at most max degree < 2^bit_length common neighbours, so every sum stays below 2^63: gl_similarity's
    64-bit sums never wrap in the driver."""
    return 62 - int(max_degree).bit_length()


def similarity_tables(degrees):
    """-> (aa uint64[n], ra uint64[n], shift): aa[w] = round(2^shift / ln(deg w)) and ra[w] = round(2^shift / deg w) where deg w
    >= 2, else 0 (a common neighbour of two distinct vertices has degree at least 2).  One f64 division and one rounding to
    nearest-even per distinct degree; the logarithm is the C library's, as in the C++ driver."""
    deg = np.asarray(degrees).astype(np.int64)
    shift = similarity_shift(int(deg.max()) if deg.size else 0)
    distinct, inverse = np.unique(deg, return_inverse=True)
    one = math.ldexp(1.0, shift)
    aa = np.array([np.rint(one / math.log(d)) if d >= 2 else 0.0 for d in distinct.tolist()], dtype=np.float64)
    ra = np.array([np.rint(one / float(d)) if d >= 2 else 0.0 for d in distinct.tolist()], dtype=np.float64)
    return aa.astype(np.uint64)[inverse].reshape(deg.shape), ra.astype(np.uint64)[inverse].reshape(deg.shape), shift


def similarity_measure(name, common, du, dv, weighted=None, shift=0):
    """-> one measure of SIMILARITY_MEASURES for pairs with `common` common neighbours and degrees du, dv, in f64 on the host
    from the integers (0.0 where a denominator is 0); `weighted` is gl_similarity's fixed-point sum for the two weighted
    measures.  common and preferential_attachment stay integers (uint32, uint64)."""
    c, a, b = np.asarray(common).astype(np.float64), np.asarray(du).astype(np.float64), np.asarray(dv).astype(np.float64)
    if name == "common":
        return np.asarray(common).astype(np.uint32)
    if name == "preferential_attachment":
        return np.asarray(du).astype(np.uint64) * np.asarray(dv).astype(np.uint64)
    if name in ("adamic_adar", "resource_allocation"):
        return np.asarray(weighted).astype(np.uint64).astype(np.float64) * math.ldexp(1.0, -shift)
    if name == "jaccard":
        num, den = c, a + b - c
    elif name == "overlap":
        num, den = c, np.minimum(a, b)
    elif name == "sorensen":
        num, den = 2.0 * c, a + b
    elif name == "cosine":
        num, den = c, np.sqrt(a * b)
    else:
        raise ValueError("similarity: unknown measure %r (one of %s)" % (name, ", ".join(SIMILARITY_MEASURES)))
    out = np.zeros(c.shape[0], dtype=np.float64)
    np.divide(num, den, out=out, where=den > 0)
    return out


def validate_similarity(csr, pairs, result):
    """Host-side check (numpy / scipy) that `result` -- the dict of Similarity.run: measure name -> array aligned with `pairs`
    (int[m, 2]) -- holds those measures on the undirected simple graph of `csr`, as Similarity reads it (io.symmetrize_simple).
    The statement is independent of the kernel's search: with S the symmetric 0/1 pattern as a scipy matrix of 64-bit integers,
    the common neighbours are the row products S[u] . S[v]^T and the weighted sums S[u] . diag(w) . S[v]^T with the fixed-point
    tables of similarity_tables (exact: every sum is below 2^63); the measures follow by similarity_measure.  Integers are
    compared exactly and the f64 values as bits.  Raises ValueError with the first violation."""
    import scipy.sparse as sp
    pr = np.asarray(pairs)
    if pr.ndim != 2 or pr.shape[1] != 2:
        raise ValueError("validate_similarity: pairs must have the shape [m, 2], not %s" % (pr.shape,))
    pr = pr.astype(np.int64)
    m = pr.shape[0]
    sym, deg = io.symmetrize_simple(csr.copy())
    n = sym.num_rows
    if m and (pr.min() < 0 or pr.max() >= n):
        raise ValueError("validate_similarity: a pair names a vertex outside 0 .. %d" % (n - 1))
    for name in result:
        if name not in SIMILARITY_MEASURES:
            raise ValueError("validate_similarity: unknown measure %r" % (name,))
        if np.asarray(result[name]).shape != (m,):
            raise ValueError("validate_similarity: %s has the shape %s for %d pairs" % (name, np.asarray(result[name]).shape, m))
    S = _pattern_as_scipy(sym, n).astype(np.int64)
    aa, ra, shift = similarity_tables(deg)
    want = {"common": np.zeros(m, np.int64), "adamic_adar": np.zeros(m, np.int64), "resource_allocation": np.zeros(m, np.int64)}
    tables = {"adamic_adar": aa, "resource_allocation": ra}
    for b in range(0, m, 1 << 16):
        u, v = pr[b:b + (1 << 16), 0], pr[b:b + (1 << 16), 1]
        Su, Sv = S[u], S[v]
        want["common"][b:b + u.shape[0]] = np.asarray(Su.multiply(Sv).sum(axis=1)).ravel()
        for name, table in tables.items():
            if name in result:
                D = sp.diags(table.astype(np.int64), dtype=np.int64, format="csr")
                want[name][b:b + u.shape[0]] = np.asarray((Su @ D).multiply(Sv).sum(axis=1)).ravel()
    du, dv = deg[pr[:, 0]], deg[pr[:, 1]]
    for name in result:
        got = np.asarray(result[name])
        exp = similarity_measure(name, want["common"], du, dv, want.get(name), shift)
        if exp.dtype == np.float64:
            bad = np.ascontiguousarray(got, dtype=np.float64).view(np.uint64) != exp.view(np.uint64)
        else:
            bad = got.astype(np.int64) != exp.astype(np.int64) if name == "common" else got.astype(np.uint64) != exp
        if np.any(bad):
            i = int(np.flatnonzero(bad)[0])
            raise ValueError("validate_similarity: pair %d = (%d, %d) has %s %r, the row product gives %r (%d common neighbours, degrees %d and %d)"
                             % (i, pr[i, 0], pr[i, 1], name, got[i].item(), exp[i].item(), want["common"][i], du[i], dv[i]))


class ModuleCollection:
    def __init__(self):
        self.modules_ = []
        self.target_ = "hw"

    def add_module(self, module):
        self.modules_.append(module)

    def set_target(self, target):
        assert target in ("sw_emu", "hw_emu", "hw")  # module_collection.h:56-59
        self.target_ = target

    def set_up_runtime(self, xclbin_file_path=None):
        """One device context for all modules (module_collection.h:69-114); the bitstream path is
        accepted for signature parity and ignored."""
        self.backend.init()
        for m in self.modules_:
            m.blocking = False


class _GraphApp(ModuleCollection):
    def __init__(self, num_channels, comm, backend):
        super().__init__()
        self.num_channels_ = num_channels
        self.comm = comm if comm is not None else Comm(None)
        self.backend = backend if backend is not None else HipBackend()
        self.bounds_ = None

    def _pad(self, csr):
        d = self.num_channels_ * M.pack_size      # app/bfs.h:86-89
        io.util_round_csr_matrix_dim(csr, d, d)

    def _load(self, src):
        return io.load_csr_matrix_from_float_npz(src) if isinstance(src, (str, bytes)) else src.copy()

    def _shard(self, csr):
        self.bounds_ = partition_rows_by_nnz(csr.adj_indptr, self.comm.world_size)
        self.r0_, self.r1_ = self.bounds_[self.comm.rank], self.bounds_[self.comm.rank + 1]

    def get_nnz(self):
        return self.SpMV_.get_nnz()

    # slice helpers -----------------------------------------------------------------------------
    def _own(self, buf):
        return self.backend.view(buf, self.r0_, self.r1_ - self.r0_, 4)

    def _gather(self, buf):
        if self.comm.distributed:
            self.comm.all_gather_slices(buf.tensor, self.bounds_)

    def _new_dense(self, n, fill, source=None, source_value=None):
        """Dense vector built on the device: a fill kernel plus (optionally) one 4-byte store, instead of
        the reference's full host-side vector + upload (e.g. app/bfs.h:107-112)."""
        B = self.backend
        buf = B.alloc(n, np.float32)
        B.fill(buf, float(fill), n)
        if source is not None:
            B.fill(B.view(buf, source, 1, 4), float(source_value), 1)   # a 1-element fill kernel: no blocking copy
        return buf

    def _gather_sparse(self, local_buf, out_buf, n, head_val):
        """All ranks contribute their (ascending, disjoint) slice of a sparse vector; every rank ends
        up with the concatenation, head {total, head_val} included.  Returns the total count."""
        B = self.backend
        cnt = self.comm_sparse_count(local_buf)
        if not self.comm.distributed:
            return cnt
        total = self.comm.all_gather_sparse(local_buf.tensor[1:], cnt, n, out_buf.tensor[1:])
        head = np.zeros(1, dtype=capi.IDX_VAL)
        head["index"][0], head["val"][0] = total, head_val
        B.upload(B.view(out_buf, 0, 1, 8), head)
        return total

    def comm_sparse_count(self, buf):
        return int(self.backend.download(buf, capi.IDX_VAL, 1)["index"][0])


class BFS(_GraphApp):
    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, spmspv_out_buf_len=0, vec_buf_len=0,
                 comm=None, backend=None):
        super().__init__(num_channels, comm, backend)
        B = self.backend
        self.semiring_ = M.LogicalSemiring
        self.SpMV_ = B.SpMVModule(num_channels, spmv_out_buf_len, vec_buf_len)
        self.SpMV_.set_semiring(self.semiring_)
        self.SpMV_.set_mask_type(M.kMaskWriteToZero)
        self.DenseAssign_ = B.AssignVectorDenseModule()
        self.DenseAssign_.set_mask_type(M.kMaskWriteToOne)
        self.SpMSpV_ = B.SpMSpVModule(spmspv_out_buf_len)
        self.SpMSpV_.set_semiring(self.semiring_)
        self.SpMSpV_.set_mask_type(M.kMaskWriteToZero)
        self.SparseAssign_ = B.AssignVectorSparseModule(False)
        self.eWiseAdd_ = B.eWiseAddModule()
        for m in (self.SpMV_, self.DenseAssign_, self.SpMSpV_, self.SparseAssign_, self.eWiseAdd_):
            self.add_module(m)
        self.gather_result_ = True      # knob: row shards all-gather the distances; False: every rank reads back its slice
        self.time_schedule_ = False     # knob: leave the schedule's GPU time alone (no read-back in it) in schedule_ms_
        self.schedule_ms_ = None        # GPU ms of the last run with time_schedule_ set
        self.readback_ = None           # the last measured read-back: {"way", "packed_ms", "float_ms"}
        self.levels_ = None             # BFS.parents(): the last run's levels on the device
        self.bits_loop_ = None          # resources of the device-resident schedule (_bits_state), per matrix
        self.results_ = self.bits_a_ = self.bits_b_ = None      # scratch of the module-call pull loop, per matrix

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True):
        csr = self._load(csr_float_npz_path)
        self._pad(csr)
        csr.adj_data = np.ones(csr.nnz, dtype=np.float32)       # app/bfs.h:90
        csc = io.csr2csc(csr)
        self._shard(csr)
        for m in (self.SpMV_, self.SpMSpV_):
            m.set_row_shard(self.r0_, self.r1_)
        self.SpMV_.load_and_format_matrix(csr, skip_empty_rows)
        self.SpMSpV_.load_and_format_matrix(csc)
        self.n_ = self.SpMV_.get_num_rows()
        assert self.n_ == self.SpMV_.get_num_cols()
        # the bit-frontier schedule takes its decisions from GLOBAL lengths (gl_bfs_bits_shard_step):
        # every rank keeps the two n-word arrays of the whole matrix
        self.row_len_ = np.diff(csr.adj_indptr.astype(np.int64)).astype(np.uint32)
        self.col_len_ = np.diff(csc.adj_indptr.astype(np.int64)).astype(np.uint32)
        self.nnz_global_ = int(csr.adj_indptr[csr.num_rows])

    def send_matrix_host_to_device(self):
        self.SpMV_.send_matrix_host_to_device()
        self.SpMSpV_.send_matrix_host_to_device()
        if hasattr(self.SpMSpV_, "attach_pull"):
            self.SpMSpV_.attach_pull(self.SpMV_)     # heavy frontiers of a push iteration go row-wise
        self.results_ = self.bits_a_ = self.bits_b_ = None   # per-matrix scratch of the pull loop
        # the device-resident schedules hold buffers sized for the old n and hipGraphs with the old plans' device
        # pointers baked in: a matrix sent again (or another one) must rebuild them
        self.bits_loop_ = None

    # -- pull ------------------------------------------------------------------------------------
    def _bind_pull(self, vector, distance):
        B, n = self.backend, self.n_
        results = self.results_     # scratch of the unfused path, kept across calls
        if results is None:
            results = self.results_ = B.alloc(n, np.float32)
        self.SpMV_.bind_vector_buf(vector)
        self.SpMV_.bind_mask_buf(distance)
        self.SpMV_.bind_results_buf(results)
        self.DenseAssign_.bind_mask_buf(self._own(vector))
        self.DenseAssign_.bind_inout_buf(self._own(distance))
        self.eWiseAdd_.bind_in_buf(self._own(results))
        self.eWiseAdd_.bind_out_buf(self._own(vector))
        # The frontier lives as BITS wherever the boolean SpMV layout allows it: row-sharded runs then exchange n/8
        # bytes per iteration instead of 4n, and on unsplit plans the whole pull iteration (masked SpMV, eWiseAdd,
        # dense assign, packing of the next frontier) is ONE launch (gl_bfs_pull_step).  Slices are whole 64-bit
        # words (shard bounds are 64-aligned).
        self.bits_ = self.bits_next_ = None
        self.fused_ = False
        self.distance_ = distance
        words = self.SpMV_.bits_words() if hasattr(self.SpMV_, "bits_words") else 0
        aligned = (not self.comm.distributed) or all(b % 64 == 0 for b in self.bounds_)
        if words and aligned:
            self.fused_ = hasattr(self.SpMV_, "fused_bfs_ok") and self.SpMV_.fused_bfs_ok()
            if self.fused_ or self.comm.distributed:
                # opaque 32-bit words, kept across calls: pack_bits / the fused step rewrite every word of the row
                # range, words past it stay 0 from the allocation
                if self.bits_a_ is None:
                    self.bits_a_, self.bits_b_ = B.alloc(words, np.float32), B.alloc(words, np.float32)
                    B.fill(self.bits_a_, 0.0, words)
                    B.fill(self.bits_b_, 0.0, words)
                self.bits_ = self.bits_a_
                capi.pack_bits(vector, n, self.bits_)
            if self.fused_:
                self.bits_next_ = self.bits_b_

    def _pull_iteration(self, vector, it):
        B, own = self.backend, self.r1_ - self.r0_
        if self.fused_:
            self.SpMV_.bfs_pull_step(self.bits_, self.bits_next_, self.distance_, float(it + 1))
            self.bits_, self.bits_next_ = self.bits_next_, self.bits_
            if self.comm.distributed:
                self.comm.all_gather_slices(self.bits_.tensor, [b // 32 for b in self.bounds_])
            return
        if self.bits_ is not None:
            self.SpMV_.run_bits(self.bits_)
        else:
            self.SpMV_.run()
        self.eWiseAdd_.run(own, 0.0)                 # results -> vector (app/bfs.h:119-122)
        self.DenseAssign_.run(own, float(it + 1))
        if self.bits_ is not None:
            capi.pack_bits(self._own(vector), own, B.view(self.bits_, self.r0_ // 32, own // 32, 4))
            self.comm.all_gather_slices(self.bits_.tensor, [b // 32 for b in self.bounds_])
        else:
            self._gather(vector)

    def _finish_distance(self, distance):
        self._gather(distance)
        self.levels_ = (distance, None)      # BFS.parents(): this run's levels, whole on every rank
        self.backend.sync()
        return self.backend.download_result(distance, self.n_)

    def pull(self, source, num_iterations):
        if self._bits_loop_ok():
            return self._pull_push_bits(source, num_iterations, -1.0, pull_only=True)
        n = self.n_
        vector = self._new_dense(n, self.semiring_.zero, source, 1.0)
        distance = self._new_dense(n, 0.0, source, 1.0)
        self._bind_pull(vector, distance)
        for it in range(1, num_iterations + 1):
            self._pull_iteration(vector, it)
        return self._finish_distance(distance)

    # -- push ------------------------------------------------------------------------------------
    def _start_push(self, source):
        B, n = self.backend, self.n_
        frontier = B.alloc(n + 1, capi.IDX_VAL)
        B.upload(B.view(frontier, 0, 2, 8), M.make_sparse_vec([source], [1.0]))
        self._hint_frontier(1)
        distance = self._new_dense(n, 0.0, source, 1.0)
        local = B.alloc(n + 1, capi.IDX_VAL)        # this rank's slice of the next frontier
        self.SpMSpV_.bind_vector_buf(frontier)
        self.SpMSpV_.bind_mask_buf(distance)
        self.SpMSpV_.results_buf = local
        self.SparseAssign_.bind_mask_buf(local)
        self.SparseAssign_.bind_inout_buf(distance)
        return frontier, distance, local

    def _hint_frontier(self, nnz):
        if hasattr(self.SpMSpV_, "hint_vector_nnz"):
            self.SpMSpV_.hint_vector_nnz(nnz)

    def _push_iteration(self, frontier, local, it):
        """SpMSpV on the shard, mark the newly reached vertices, publish the next frontier.  Returns
        (frontier size, frontier buffer, result buffer) for the next iteration."""
        # SpMSpV, then distance[new] = level (app/bfs.h:146-148); the assign rides on the pass that writes the results
        if hasattr(self.SpMSpV_, "run_assign"):
            self.SpMSpV_.run_assign(self.SparseAssign_.inout_buf, float(it + 1))
        else:
            self.SpMSpV_.run()
            self.SparseAssign_.run(float(it + 1))
        if self.comm.distributed:
            total = self._gather_sparse(local, frontier, self.n_, self.semiring_.zero)
            self._hint_frontier(total)
            return total, frontier, local
        nnz = self.SpMSpV_.get_results_nnz()
        # the reference copies results -> vector here (app/bfs.h:149-152); the two buffers swap roles instead
        frontier, local = local, frontier
        self.SpMSpV_.bind_vector_buf(frontier)
        self.SpMSpV_.results_buf = local
        self.SparseAssign_.bind_mask_buf(local)
        self._hint_frontier(nnz)
        return nnz, frontier, local

    def push(self, source, num_iterations):
        frontier, distance, local = self._start_push(source)
        for it in range(1, num_iterations + 1):
            _, frontier, local = self._push_iteration(frontier, local, it)
        return self._finish_distance(distance)

    # -- pull / pull_push without the host in the loop ------------------------------------------
    def _pull_push_bits(self, source, num_iterations, threshold, pull_only=False):
        """The reference decides push vs pull on the host from a count it reads back every iteration (app/bfs.h:180-190) and
        converts the frontier on the host at the switch (:195-205).  Here the WHOLE run is enqueued up front as a device-resident
        schedule with the frontier as BITS only (gl_bfs_bits_shard_step, csrc/gl_bfs_shard.h): ONE launch per iteration slot --
        it begins with the previous slot's decision (the reference's loop condition, replayed from the slot's tallies) and then
        runs the step the state asks for: the scattering push straight into the next frontier's bit vector, the streaming
        (||,&&) pull, which also serves a push whose frontier is heavy, or the bottom-up scan of the rows not reached yet.
        Slot s reads bit vector s and writes vector s + 1.  No synchronisation and no device->host copy between the first
        launch and the read-back; the schedule depends only on (iterations, threshold) -- the source is a device word -- so it
        is recorded once as a hipGraph and replayed.  (pull_only: BFS.pull, app/bfs.h:106-126 -- no slot scatters.)

        ROW SHARDS (comm.distributed) run the same launches on their rows; ONE all-gather per slot rebuilds the slot's bit
        vector (n/8 bytes) and carries every rank's tallies (256 bytes each), from which every rank takes the same decision;
        every rank reads back ITS SLICE of the distances (`gather_result_` = True all-gathers them first).

        What remains beside this schedule is the reference's own module-call loop (GRAPHLILY_BFS_HOST_LOOP=1, and wherever the
        plans do not offer the bit layout); the earlier generations of this loop: EXPERIMENTS.md R4.3.

        The phases, in the order they run: _bits_state, _emulation_inputs, _result_range, _readback_plan, _levels_block,
        _launch_or_replay (_enqueue_bits_schedule, _enqueue_packed_levels), _gather_distances, _fetch_levels, _record_readback,
        _publish_ctl."""
        N, timed = num_iterations, self.time_schedule_
        self.fused_ = True          # (every pull step of this schedule is the fused one, see _bind_pull)
        st = self._bits_state(N)
        gathered, tally_in = self._emulation_inputs(st, source, N)
        # Once the reference's rule has switched to pulling (frontier / n >= threshold, app/bfs.h:180-190), every later slot is
        # handed back to the push step (an extension: the reference pulls to the end), which leaves heavy frontiers to the
        # streaming pull anyway: from then on the direction follows the work.  Distances do not depend on the direction.
        back = 0.0 if pull_only else 1.0
        sliced, lo, hi = self._result_range()
        book = st["readback"][BookKey(N, float(threshold), back, pull_only, lo, hi - lo)]
        plan = self._readback_plan(N, lo, hi, sliced, timed, book)
        t_call = time.perf_counter()
        self._levels_block(st, plan)
        capi.fill_u32(self.backend.view(st["ctl"], capi.GL_BFS_CTL_SOURCE, 1, 4), int(source), 1)   # (a device word: replays take any source)
        key = GraphKey(N, float(threshold), back, pull_only, plan.in_graph, lo, plan.own)
        enqueue = functools.partial(self._enqueue_bits_schedule, st, N, threshold, pull_only, back, gathered, tally_in)
        replayed = self._launch_or_replay(st, key, enqueue, functools.partial(self._enqueue_packed_levels, st, plan))
        if not sliced:
            self._gather_distances(st)
        res, c = self._fetch_levels(st, plan, replayed)
        if plan.can_pack and not timed:
            self._record_readback(book, plan, time.perf_counter() - t_call)
        self.result_range_ = (lo, hi)
        # BFS.parents(): this run's levels stay in the schedule's buffer (a rank that read back only its slice holds only its
        # rows of them: parents() all-gathers first)
        # (plain handles, no closure over self: a reference cycle would leave the driver's plans and buffers to the garbage collector)
        self.levels_ = (st["distance"], st["both"] if sliced else None)
        self._publish_ctl(c, N, st["ctl_words"])
        return res

    def _result_range(self):
        """-> (sliced, lo, hi): a row shard with `gather_result_` off reads back its own rows [lo, hi) only."""
        sliced = self.comm.distributed and not self.gather_result_
        return (sliced, self.r0_, self.r1_) if sliced else (sliced, 0, self.n_)

    def _gather_distances(self, st):
        """Row shards: every rank's rows of the distances to every rank, behind the schedule."""
        if self.comm.distributed:
            both = st["both"]
            self.comm.all_gather_slices(both.tensor[:self.n_] if both.tensor is not None else both, self.bounds_)

    def _record_readback(self, book, plan, seconds):
        """A whole call that could have gone either way is a measurement of the way it went."""
        way = "packed" if plan.as_bytes else "float"
        book.record(way, seconds)
        self.readback_ = book.report(way)

    def _bits_state(self, N):
        """self.bits_loop_, built on the first run and again when a run needs more slots than it has (send_matrix_host_to_device
        drops it).  A plain dict of resources:
          N, nvec, nvec_all, words, ctl_words   slots it serves; bit vectors (N + 2), those plus the room of the tallies; 32-bit
                                                words of a bit vector and of the control words
          both, distance, ctl                   n distances and the control words behind them (one read-back fetches both); views
          vecs, bits, tally                     the bit vectors in one allocation; a view of each; the ranks' tallies behind them
                                                (gl_bfs_bits_shard_step), cleared with them
          col_len, row_len                      the GLOBAL column (and, row-sharded, row) lengths on the device
          graphs, warm, graph_error             GraphKey -> recorded hipGraph (False: capture failed, the message is in
                                                graph_error); the keys enqueued once
          readback                              the packed-or-float books: BookKey -> readback.ReadbackBook
          lev8_key, lev8, h8                    (_levels_block) the packed read-back's device and page-locked blocks"""
        st = self.bits_loop_
        if st is not None and st["N"] >= N:
            return st
        B, n = self.backend, self.n_
        words = (int(self.SpMV_.bits_words()) + 3) & ~3
        nvec, ctl_words = N + 2, (18 + 2 * N + 15) & ~15
        both = B.alloc(n + ctl_words, np.float32)
        tally_words = capi.bfs_tally_words(N, self.comm.world_size)
        nvec_all = nvec + (tally_words + words - 1) // words
        vecs = B.alloc(nvec_all * words, np.float32)
        st = self.bits_loop_ = {"N": N, "both": both, "vecs": vecs, "words": words, "nvec": nvec, "ctl_words": ctl_words,
                                "ctl": B.view(both, n, ctl_words, 4), "distance": B.view(both, 0, n, 4),
                                "bits": [B.view(vecs, k * words, words, 4) for k in range(nvec)], "graphs": {},
                                "warm": set(), "nvec_all": nvec_all, "readback": collections.defaultdict(ReadbackBook)}
        st["col_len"] = capi.DeviceBuffer.from_host(self.col_len_)
        st["tally"] = B.view(vecs, nvec * words, tally_words, 4)
        if self.comm.distributed:
            st["row_len"] = capi.DeviceBuffer.from_host(self.row_len_)
        return st

    def _emulation_inputs(self, st, source, N):
        """-> (the bit vectors the slots read, the tally table they read).  A real run reads its own: (st["bits"], None).  The
        one-GPU emulation of a rank (dist.EmulatedComm) has the whole run's tallies computed, and without an exchange step
        (copy=False) its slots read the whole run's vectors and tallies."""
        comm = self.comm
        if not getattr(comm, "emulated", False):
            return st["bits"], None
        table = comm.truth_tally((source, N), N, self.bounds_, self.col_len_, self.row_len_, self.n_)
        if comm.copy:
            return st["bits"], None
        return [comm.truth_vector(k) for k in range(st["nvec"])], table

    def _enqueue_bits_schedule(self, st, N, threshold, pull_only, back, gathered, tally_in):
        """The launches of one run: begin, one step per slot (and its exchange, row-sharded), finish."""
        ctl, distance, bits, words, tally, col_len = st["ctl"], st["distance"], st["bits"], st["words"], st["tally"], st["col_len"]
        csc_plan, pull_plan, nnz = self.SpMSpV_.plan_, self.SpMV_.plan_, self.nnz_global_
        rank, world, sharded = self.comm.rank, self.comm.world_size, self.comm.distributed

        def may_of(it):
            return (1 if it + 1 < N else 0) | (2 if it + 1 <= N else 0)

        capi.bfs_bits_begin(ctl, st["ctl_words"], distance, self.n_, st["vecs"], words, st["nvec_all"], 0 if pull_only else 0xffffffff)
        for it in range(1, N + 1):
            capi.bfs_bits_shard_step(csc_plan, pull_plan, gathered[it], bits[it + 1], words, distance, float(it + 1), ctl, tally,
                                     tally_in, it, rank, world, col_len, nnz, threshold, may_of(it - 1) if it > 1 else 0, back)
            if sharded:
                self._exchange_bits(st, it + 1, it)
        capi.bfs_bits_shard_finish(csc_plan, pull_plan, ctl, tally, tally_in, N, rank, world, nnz, threshold, may_of(N), back)

    def _readback_plan(self, N, lo, hi, sliced, timed, book):
        """How this call's levels [lo, hi) come back.  Levels are small integers: when they fit a byte (N + 1 <= 255; a nibble up
        to 14 iterations) the result can cross PCIe PACKED -- 1.5 or 3 MB instead of 12 MB on orkut, 28 or 55 us instead of 225,
        the control words behind them in the same copy -- and a few host threads turn them into the floats the caller gets
        (woken while the GPU is still busy).  The packed way is possible (can_pack) from half a million rows on: in a
        same-machine A/B (profiles/r04_ab_schedules.txt) the googleplus stand-in's 108 K levels, 0.43 MB as floats, came back
        24 us SOONER unpacked, ogbl-ppa's 576 K tie, hollywood's 1 M gain 22 us packed.  Where it is possible, `book` (this
        schedule's readback.ReadbackBook) chooses between packed and floats from what it has measured (as_bytes);
        GRAPHLILY_BFS_U8=0 / =2 pin the float / packed way.  The pack is part of the recorded schedule (fixed buffers) unless
        the schedule's GPU time alone is wanted, or the distances are all-gathered first.  The pack kernel stores into the
        page-locked block itself, chunk by chunk with a flag behind each, and the host threads expand a chunk as soon as it has
        landed -- the expansion overlaps the PCIe transfer (GRAPHLILY_BFS_STREAM=0: pack -> copy -> wait -> expand)."""
        own = hi - lo
        pin = os.environ.get("GRAPHLILY_BFS_U8", "1")
        can_pack = (N + 1 <= 255 and own % 8 == 0 and lo % 4 == 0 and own >= (1 << 19)
                    and pin != "0" and capi.host_unpack_threads() >= 4)
        as_bytes = book.choose(can_pack, timed, pin)
        in_graph = as_bytes and not timed and (sliced or not self.comm.distributed)
        streamed = as_bytes and os.environ.get("GRAPHLILY_BFS_STREAM", "1") != "0"
        return ReadbackPlan(lo, hi, own, 4 if N + 1 <= 15 else 8, can_pack, as_bytes, streamed, in_graph)

    def _levels_block(self, st, plan):
        """The blocks a packed read-back lands in, kept while (own, bits per level, streamed) stay: a change drops the graphs
        that recorded the old ones.  A streamed block is armed here: before anything of this run is launched."""
        if not plan.as_bytes:
            return
        own, pbits, streamed, cw = plan.own, plan.pbits, plan.streamed, st["ctl_words"]
        if st.get("lev8_key") != (own, pbits, streamed):
            nbytes = 4 * (capi.levels_packed_words(own, pbits) + cw)
            st["lev8_key"] = (own, pbits, streamed)
            st["lev8"] = None if streamed else capi.DeviceBuffer(nbytes)
            st["h8"] = capi.pinned_empty(capi.levels_stream_bytes(own, pbits, cw) if streamed else nbytes, np.uint8)
            st["graphs"] = {k: g for k, g in st["graphs"].items() if not k.packed_read_back}
        if streamed:
            capi.levels_stream_arm(st["h8"], own, pbits, cw)

    def _enqueue_packed_levels(self, st, plan):
        """The device half of the packed read-back: levels [lo, hi), then the control words, into the page-locked block."""
        levels, cw = self.backend.view(st["distance"], plan.lo, plan.own, 4), st["ctl_words"]
        if plan.streamed:
            capi.levels_pack_stream(levels, plan.own, plan.pbits, st["ctl"], cw, st["h8"])
            return
        capi.levels_pack(levels, plan.own, plan.pbits, st["ctl"], cw, st["lev8"])
        st["lev8"].read_async(st["h8"])

    def _launch_or_replay(self, st, key, enqueue, enqueue_levels):
        """The schedule of `key` (`enqueue()`; key.packed_read_back: `enqueue_levels()` behind it in the recording): enqueued on
        the first call, recorded as a hipGraph on the second, replayed from then on.  -> whether a graph ran.  With
        `time_schedule_` the run's GPU time is left in `schedule_ms_`."""
        timed = self.time_schedule_
        g = st["graphs"].get(key)
        # (a torch.distributed collective is not recorded by the library's capture: those runs are enqueued call by call)
        capturable = not self.comm.distributed or getattr(self.comm, "capturable", False)
        if g is None and capturable and key in st["warm"]:
            try:
                with capi.Graph.capture() as g:
                    enqueue()
                    if key.packed_read_back:
                        enqueue_levels()
                st["graphs"][key] = g
            except capi.GraphLilyError as e:
                g = st["graphs"][key] = False              # capture not possible here: keep enqueueing
                st["graph_error"] = str(e)
        if timed:
            capi.span_begin()
        if g:
            g.launch()
        else:
            enqueue()
            st["warm"].add(key)
        if timed:
            self.schedule_ms_ = capi.span_end()
        return bool(g)

    def _fetch_levels(self, st, plan, replayed):
        """Waits for the run.  -> (levels [lo, hi) as floats, the control words as uint32)."""
        own, cw = plan.own, st["ctl_words"]
        if not plan.as_bytes:
            # the distances (this rank's slice of them) + the control words: two copies behind the schedule, one wait
            n, out = self.n_, capi.pinned_recycled(own + cw, np.float32)
            if own == n:
                st["both"].read_async(out)                    # (the control words follow the distances: one copy)
            else:
                st["both"].read_async(out[:own], 4 * plan.lo)
                st["both"].read_async(out[own:], 4 * n)
            self.backend.sync()
            return out[:own], out[own:].view(np.uint32)
        if not (replayed and plan.in_graph):
            self._enqueue_packed_levels(st, plan)
        res = capi.pinned_recycled(own, np.float32)       # (recycled: already paged in)
        if plan.streamed:
            return res, capi.sync_levels_unpack_stream(res, st["h8"], own, plan.pbits, cw)   # (the host threads start now: chunk by chunk)
        capi.sync_levels_unpack(res, st["h8"], own, plan.pbits)   # (the host threads start now and spin until the stream is done)
        return res, st["h8"][4 * capi.levels_packed_words(own, plan.pbits):].view(np.uint32).copy()

    def _publish_ctl(self, c, N, ctl_words):
        """The run's books from its control words (capi.GL_BFS_CTL_*)."""
        counts = capi.GL_BFS_CTL_HEAD_WORDS + 1               # (slots are numbered from 1)
        modes = counts + capi.bfs_ctl_slots(ctl_words)
        self.push_iterations_ = int(c[capi.GL_BFS_CTL_PUSHES])                # the reference's count (first push phase)
        self.push_iterations_again_ = int(c[capi.GL_BFS_CTL_PUSHES_AGAIN])    # pushes after a pull step handed back
        self.bfs_slot_counts_ = c[counts:counts + N].copy()      # vertices reached per slot
        self.bfs_slot_modes_ = c[modes:modes + N].copy()         # 1 scattered, 2 streamed row-wise, 3 bottom-up, 0 nothing ran

    def _exchange_bits(self, st, k, tally_slot):
        """The one exchange step of a sharded slot: every rank's rows of bit vector k to every rank, and every rank's tallies
        of slot `tally_slot` (256 bytes each) along with them."""
        comm, W = self.comm, self.comm.world_size
        per = capi.GL_BFS_TALLY_RANK_WORDS
        first = capi.GL_BFS_TALLY_HEAD_WORDS + (tally_slot - 1) * W * per
        if hasattr(comm, "exchange_bits"):                 # the C-ABI communicator (gl_dist_*) or the one-GPU emulation
            comm.exchange_bits(st["bits"][k], k, self.bounds_, self.backend.view(st["tally"], first, W * per, 4), tally_slot)
            return
        t = st["vecs"].tensor[k * st["words"]:(k + 1) * st["words"]]
        base = st["nvec"] * st["words"] + first               # ONE collective per slot: the tallies ride behind the rank's bits
        comm.all_gather_slices_with_tail(t, [b // 32 for b in self.bounds_], st["vecs"].tensor[base:base + W * per], per)

    def _bits_loop_ok(self):
        """Can this BFS run as the device-resident schedule?  (GRAPHLILY_BFS_HOST_LOOP=1: no -- the reference's loop.)"""
        if os.environ.get("GRAPHLILY_BFS_HOST_LOOP", "0") != "0" or not hasattr(capi, "bfs_bits_shard_step"):
            return False
        if getattr(self.SpMV_, "plan_", None) is None or getattr(self.SpMSpV_, "plan_", None) is None:
            return False
        if not (hasattr(self.SpMV_, "bits_words") and self.SpMV_.bits_words() > 0 and self.SpMV_.semiring_.zero == 0.0):
            return False
        if self.comm.distributed:      # any boolean plan whose row range is cut on multiples of 64 rows
            return all(b % 64 == 0 for b in self.bounds_[:-1])
        return hasattr(self.SpMV_, "fused_bfs_ok") and self.SpMV_.fused_bfs_ok()

    def pull_push(self, source, num_iterations, threshold=0.05):
        if self._bits_loop_ok():
            return self._pull_push_bits(source, num_iterations, threshold)
        n = self.n_
        frontier, distance, local = self._start_push(source)
        it = 1
        while True:
            nnz, frontier, local = self._push_iteration(frontier, local, it)
            it += 1
            if not (it < num_iterations and float(nnz) / n < threshold):
                break
        self.push_iterations_ = it - 1
        # switch: the frontier becomes the dense SpMV input (app/bfs.h:195-205), on the device
        vector = self.backend.alloc(n, np.float32)
        self.backend.sparse_to_dense(frontier, vector, n, M.LogicalSemiring.zero, n)
        self._bind_pull(vector, distance)
        while it <= num_iterations:
            self._pull_iteration(vector, it)
            it += 1
        return self._finish_distance(distance)


    # -- predecessor tree (an extension: the reference's drivers return levels only) ------------------------------------------
    def parents(self, distance=None):
        """The BFS predecessor tree as uint32[n]: parent[v] = v on the source (level 1), NO_PARENT (0xffffffff) on an unreached
        vertex (level 0), otherwise the SMALLEST u with an entry A[v, u] != 0 and level[u] == level[v] - 1 -- unique, whichever
        mix of push / pull / bottom-up steps found the levels.  One pass over the rows from the finished level vector
        (gl_bfs_parents): `distance=None` takes the levels of this object's last pull / push / pull_push, which are still on the
        device; an array (n floats, the drivers' levels) is uploaded and used instead.  Row shards compute their own rows from
        the whole level vector and all-gather the slices.  `orphans_` = vertices of level >= 2 without such a u among this
        rank's rows (0 for a BFS result)."""
        B, n = self.backend, self.n_
        if distance is None:
            last = self.levels_
            if last is None:
                raise RuntimeError("BFS.parents(): no pull / push / pull_push has run on this object; pass the level array")
            levels, partial = last
            if partial is not None:      # the schedule's buffer of a rank that read back only its slice
                self.comm.all_gather_slices(partial.tensor[:n] if partial.tensor is not None else partial, self.bounds_)
        else:
            arr = np.ascontiguousarray(distance, dtype=np.float32)
            if arr.shape != (n,):
                raise ValueError("BFS.parents(): the level array has shape %s, the (padded) matrix has %d rows" % (arr.shape, n))
            levels = B.alloc(n, np.float32)
            B.upload(levels, arr)
        par = B.alloc(n + 1, np.float32)      # (32-bit words: vertex numbers, then the orphan count)
        self.SpMV_.bfs_parents(levels, self._own(par), B.view(par, n, 1, 4))
        self._gather(par)
        B.sync()
        out = B.download(par, np.uint32, n + 1)
        self.orphans_ = int(out[n])
        return out[:n]

    def pull_push_time_breakdown(self, source, num_iterations, threshold=0.05):
        """app/bfs.h:222-347: pull_push with the reference's four wall-clock buckets.  Every step is followed by
        a device sync (the reference's module calls are blocking), so the total is larger than pull_push's.
        Returns the same distance vector; the buckets (ms) are left in `time_breakdown_` and printed."""
        B, n = self.backend, self.n_
        tb = {"spmv_spmspv": 0.0, "assign": 0.0, "data_transfer": 0.0}

        def timed(bucket, fn):
            B.sync()
            t0 = time.perf_counter()
            r = fn()
            B.sync()
            tb[bucket] += (time.perf_counter() - t0) * 1e3
            return r

        B.sync()
        t_start = time.perf_counter()
        frontier, distance, local = timed("data_transfer", lambda: self._start_push(source))
        it = 1
        while True:
            timed("spmv_spmspv", self.SpMSpV_.run)
            timed("assign", lambda: self.SparseAssign_.run(float(it + 1)))
            if self.comm.distributed:
                nnz = timed("data_transfer", lambda: self._gather_sparse(local, frontier, n, self.semiring_.zero))
            else:
                nnz = self.SpMSpV_.get_results_nnz()
                timed("data_transfer", lambda: B.copy(frontier, local, 8 * (1 + nnz)))
            self._hint_frontier(nnz)
            it += 1
            if not (it < num_iterations and float(nnz) / n < threshold):
                break
        self.push_iterations_ = it - 1
        print("SpMSpV runs for %d iterations" % (it - 1))
        vector = B.alloc(n, np.float32)
        timed("data_transfer", lambda: B.sparse_to_dense(frontier, vector, n, M.LogicalSemiring.zero, n))
        self._bind_pull(vector, distance)
        own = self.r1_ - self.r0_
        while it <= num_iterations:
            timed("spmv_spmspv", self.SpMV_.run)
            timed("data_transfer", lambda: (self.eWiseAdd_.run(own, 0.0), self._gather(vector)))
            timed("assign", lambda: self.DenseAssign_.run(own, float(it + 1)))
            it += 1
        result = timed("data_transfer", lambda: self._finish_distance(distance))
        total = (time.perf_counter() - t_start) * 1e3
        tb["total"] = total
        tb["overhead"] = total - tb["spmv_spmspv"] - tb["assign"] - tb["data_transfer"]
        self.time_breakdown_ = tb
        for k in ("total", "spmv_spmspv", "assign", "data_transfer", "overhead"):
            print("%s_time_ms: %.4f" % (k, tb[k]))
        return result


class _PatternApp(_GraphApp):
    """What the single-device drivers of the kernels that walk a boolean plan's plain row copy share (extensions: the reference
    has no such drivers): one SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, which keeps that
    copy; a matrix that _prepare() turns into what the kernel accepts; no row shards, for the reason _no_shards_ gives."""
    _no_shards_ = ""

    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, vec_buf_len=0, comm=None, backend=None):
        _GraphApp.__init__(self, num_channels, comm, backend)
        self._refuse_shards()
        self.semiring_ = M.LogicalSemiring
        self.SpMV_ = self.backend.SpMVModule(num_channels, spmv_out_buf_len, vec_buf_len)
        self.SpMV_.set_semiring(self.semiring_)
        self.SpMV_.set_mask_type(M.kNoMask)
        self.add_module(self.SpMV_)
        self.sent_ = False

    def _refuse_shards(self):
        if self.comm.distributed:                                # (called before anything touches the device)
            raise NotImplementedError("%s: row shards are not supported -- %s" % (type(self).__name__, self._no_shards_))

    def _require_sent(self):
        if not self.sent_:
            raise RuntimeError("%s.run(): send_matrix_host_to_device first" % type(self).__name__)

    def _prepare(self, csr):
        """-> the matrix to plan, from the padded one (padding vertices have empty rows)"""
        return csr

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True):
        csr = self._load(csr_float_npz_path)
        self.n_real_ = csr.num_rows
        self._pad(csr)
        csr = self._prepare(csr)
        self._shard(csr)
        self.SpMV_.set_row_shard(self.r0_, self.r1_)
        self.SpMV_.load_and_format_matrix(csr, skip_empty_rows)
        self.n_ = self.SpMV_.get_num_rows()
        assert self.n_ == self.SpMV_.get_num_cols()
        self.sent_ = False

    def send_matrix_host_to_device(self):
        self.SpMV_.send_matrix_host_to_device()
        self.sent_ = True

    def _peel_order(self):
        """-> (uint32[n_], int): gl_kcore on the same plan: a degeneracy ordering of the vertices -- what the "smallest_last"
        colouring order is made of -- and the degeneracy.  The call waits for the device."""
        B, n = self.backend, self.n_
        peel = B.alloc(2 * n, np.float32)                            # (32-bit words: the core numbers, then the order)
        degeneracy = self.SpMV_.kcore(B.view(peel, 0, n, 4), B.view(peel, n, n, 4))[0]
        B.sync()
        return B.download(peel, np.uint32, 2 * n)[n:], degeneracy


class _WeightedPatternApp(_PatternApp):
    """... and of those whose kernels take a weight per entry: _prepare() leaves the symmetric weighted matrix in graph_, with
    the weights in adj_data, and returns _ones_of_graph(), because the row copy would store a zero value as no entry; the
    weights travel in a buffer of their own, aligned with graph_.adj_indices."""
    degrees_ = graph_ = weight_buf_ = edges_ = weights_ = total_weight_ = None

    def _ones_of_graph(self):
        self.weight_buf_ = None
        g = self.graph_
        return io.CSRMatrix(g.num_rows, g.num_cols, np.ones(g.nnz, dtype=np.float32), g.adj_indices, g.adj_indptr)

    def send_matrix_host_to_device(self):
        _PatternApp.send_matrix_host_to_device(self)
        self.weight_buf_ = self.backend.alloc(max(1, self.graph_.nnz), np.float32)
        if self.graph_.nnz:
            self.backend.upload(self.weight_buf_, self.graph_.adj_data)

    def _collect_edges(self, chosen):
        """-> bool[graph_.nnz]: chosen(rows, cols) over the entries of graph_.  Leaves edges_ (int64[m, 2]: (lo, hi) of every
        chosen edge, once, ascending), weights_ (float32[m], aligned with edges_) and total_weight_ (their f64 sum in that
        order)."""
        rows = np.repeat(np.arange(self.n_, dtype=np.int64), np.diff(self.graph_.adj_indptr.astype(np.int64)))
        cols = self.graph_.adj_indices.astype(np.int64)
        mask = chosen(rows, cols)
        once = np.flatnonzero(mask & (cols > rows))
        self.edges_ = np.stack([rows[once], cols[once]], axis=1)
        self.weights_ = self.graph_.adj_data[once]
        self.total_weight_ = float(np.cumsum(self.weights_, dtype=np.float64)[-1]) if once.size else 0.0     # (cumsum: one by one, in order)
        return mask


class ConnectedComponents(_PatternApp):
    """Weakly connected components: gl_cc_labels, lock-free union-find over the rows, then pointer doubling.
    run() labels every vertex with the smallest vertex of its component."""
    _no_shards_ = ("every rank would hold the forest of its own rows and the forests would have to be merged.  On ONE device "
                   "gl_cc_hook composes: cc_begin, cc_hook on every shard's plan, cc_finish (capi.cc_begin / SpMVPlan.cc_hook / "
                   "capi.cc_finish)")
    num_components_ = largest_component_ = None

    def _prepare(self, csr):
        csr.adj_data = np.ones(csr.nnz, dtype=np.float32)       # every stored entry is an edge, as in BFS (app/bfs.h:90)
        return csr

    def run(self):
        """-> uint32[n_]: labels[v] = the smallest vertex joined to v by a chain of stored entries taken in either direction
        (padding vertices are singletons).  Leaves num_components_ (over the n_real_ real vertices) and largest_component_
        (vertices in the largest one)."""
        self._require_sent()
        B, n = self.backend, self.n_
        out = B.alloc(n + 1, np.float32)      # (32-bit words: vertex numbers, then the component count)
        self.SpMV_.cc_labels(out, B.view(out, n, 1, 4))
        B.sync()
        words = B.download(out, np.uint32, n + 1)
        labels = words[:n]
        self.num_components_ = int(words[n]) - (n - self.n_real_)
        self.largest_component_ = int(np.bincount(labels, minlength=1).max()) if n else 0
        return labels


class TriangleCount(_PatternApp):
    """Triangle counting: gl_tc_count.  The matrix is read as an undirected simple graph -- duplicates, the
    diagonal, zero-valued entries and direction are ignored, as in ConnectedComponents -- and oriented by degree on the host
    (io.triangle_orient), so that every triangle is found exactly once and hub rows are short."""
    _no_shards_ = "gl_tc_count reads row u for every column u of a row, so every rank would need the whole oriented matrix"
    degrees_ = num_triangles_ = triangles_ = num_wedges_ = transitivity_ = None

    def _prepare(self, csr):
        csr, self.degrees_ = io.triangle_orient(csr)
        return csr

    def run(self, per_vertex=True):
        """-> uint64[n_]: triangles[v] = triangles through v (padding vertices: 0); with per_vertex=False -> the number of
        triangles as an int (a kernel without the per-vertex bookkeeping).  Leaves num_triangles_, triangles_ (None for a
        total-only run), num_wedges_ = sum of deg (deg - 1) / 2 and transitivity_ = 3 triangles / wedges (0.0 without wedges)."""
        self._require_sent()
        B, n = self.backend, self.n_
        words = n + 1 if per_vertex else 1
        out = B.alloc(2 * words, np.float32)      # (64-bit words: the total, then the per-vertex counts)
        self.SpMV_.tc_count(B.view(out, 0, 1, 8), B.view(out, 1, n, 8) if per_vertex else None)
        B.sync()
        got = B.download(out, np.uint64, words)
        self.num_triangles_ = int(got[0])         # (the orientation gives every triangle once)
        self.triangles_ = got[1:] if per_vertex else None
        deg = self.degrees_.astype(np.int64)
        self.num_wedges_ = sum(int(d) * (int(d) - 1) // 2 * int(c) for d, c in zip(*np.unique(deg, return_counts=True)))
        self.transitivity_ = 3.0 * self.num_triangles_ / self.num_wedges_ if self.num_wedges_ else 0.0
        return self.triangles_ if per_vertex else self.num_triangles_

    def clustering(self):
        """-> float64[n_]: the local clustering coefficient 2 t[v] / (deg[v] (deg[v] - 1)) of the last per-vertex run, 0 where
        deg[v] < 2"""
        if self.triangles_ is None:
            raise RuntimeError("TriangleCount.clustering(): run(per_vertex=True) first")
        deg = self.degrees_.astype(np.float64)
        pairs = deg * (deg - 1.0)
        out = np.zeros(self.n_, dtype=np.float64)
        np.divide(2.0 * self.triangles_.astype(np.float64), pairs, out=out, where=pairs > 0)
        return out


class KCore(_PatternApp):
    """k-core decomposition: gl_kcore.  The matrix is read as an undirected simple graph -- duplicates, the
    diagonal, zero-valued entries and direction are ignored, as in TriangleCount -- and stored in both directions by the host
    (io.symmetrize_simple): peeling v must reach every neighbour of v through row v."""
    _no_shards_ = "gl_kcore reads row u for every column u of a row, so every rank would need the whole symmetric matrix"
    degrees_ = core_ = order_ = degeneracy_ = levels_ = sub_rounds_ = launches_ = core_sizes_ = None

    def _prepare(self, csr):
        csr, self.degrees_ = io.symmetrize_simple(csr)
        return csr

    def run(self, order=False):
        """-> uint32[n_]: core[v] = the core number of v (padding vertices: 0).  Leaves core_, degeneracy_ = max core, order_
        (uint32[n_], a degeneracy ordering -- not unique -- or None without order=True), levels_ (levels that peeled a vertex,
        padding vertices included), sub_rounds_, launches_ and core_sizes_[k] = real vertices with core >= k, k = 0 ..
        degeneracy_.  The call waits for the device."""
        self._require_sent()
        B, n = self.backend, self.n_
        out = B.alloc(2 * n if order else n, np.float32)          # (32-bit words: the core numbers, then the order)
        stats = self.SpMV_.kcore(B.view(out, 0, n, 4), B.view(out, n, n, 4) if order else None)
        B.sync()
        got = B.download(out, np.uint32, 2 * n if order else n)
        self.core_ = got[:n]
        self.order_ = got[n:] if order else None
        self.degeneracy_, self.levels_, self.sub_rounds_, self.launches_ = stats
        counts = np.bincount(self.core_[:self.n_real_], minlength=self.degeneracy_ + 1)
        self.core_sizes_ = np.cumsum(counts[::-1])[::-1].astype(np.int64)
        return self.core_

    def k_core(self, k):
        """-> bool[n_]: the vertices of the k-core of the last run (core number >= k); padding vertices are in none"""
        if self.core_ is None:
            raise RuntimeError("KCore.k_core(): run() first")
        mask = self.core_ >= k
        mask[self.n_real_:] = False
        return mask


class KTruss(_PatternApp):
    """k-truss decomposition: gl_truss, the edge-wise counterpart of KCore.  The matrix is read as an undirected
    simple graph -- duplicates, the diagonal, zero-valued entries and direction are ignored, as in KCore -- and stored in both
    directions by the host (io.symmetrize_simple); that matrix is kept as graph_, and every result has one word per ENTRY of it,
    aligned with graph_.adj_indices: both entries of an edge carry the same value."""
    _no_shards_ = "gl_truss reads row u for every column u of a row, so every rank would need the whole symmetric matrix"
    degrees_ = graph_ = truss_ = support_ = max_truss_ = levels_ = sub_rounds_ = launches_ = None
    num_edges_ = num_triangles_ = truss_sizes_ = vertex_truss_ = None

    def _prepare(self, csr):
        csr, self.degrees_ = io.symmetrize_simple(csr)
        self.graph_ = csr
        self.truss_ = None
        return csr

    def run(self, support=False):
        """-> uint32[graph_.nnz]: truss[j] = the truss number of the edge of entry j (at least 2).  Leaves truss_, support_
        (uint32[graph_.nnz], the triangles through every entry's edge, or None without support=True), max_truss_ (0 for a graph
        without edges), levels_ (distinct truss numbers), sub_rounds_, launches_, num_edges_, num_triangles_, truss_sizes_[k] =
        edges with truss >= k, k = 0 .. max_truss_, and vertex_truss_ (uint32[n_]: the largest truss number among a vertex's
        edges, 0 if it has none).  The call waits for the device."""
        self._require_sent()
        B, n, nnz = self.backend, self.n_, self.graph_.nnz
        out = B.alloc(max(1, 2 * nnz if support else nnz), np.float32)   # (32-bit words: the truss numbers, then the supports)
        stats = self.SpMV_.truss(B.view(out, 0, max(1, nnz), 4), B.view(out, nnz, nnz, 4) if support and nnz else None)
        B.sync()
        got = B.download(out, np.uint32, 2 * nnz if support else nnz) if nnz else np.zeros(0, np.uint32)
        self.truss_ = got[:nnz]
        self.support_ = got[nnz:] if support else None
        self.max_truss_, self.levels_, self.sub_rounds_, self.launches_, self.num_edges_, self.num_triangles_ = stats
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.graph_.adj_indptr.astype(np.int64)))
        once = self.graph_.adj_indices.astype(np.int64) > rows
        counts = np.bincount(self.truss_[once], minlength=self.max_truss_ + 1)
        self.truss_sizes_ = np.cumsum(counts[::-1])[::-1].astype(np.int64)
        self.vertex_truss_ = np.zeros(n, dtype=np.uint32)
        np.maximum.at(self.vertex_truss_, rows, self.truss_)
        return self.truss_

    def k_truss(self, k):
        """-> bool[graph_.nnz]: the entries of the k-truss of the last run (truss number >= k)"""
        if self.truss_ is None:
            raise RuntimeError("KTruss.k_truss(): run() first")
        return self.truss_ >= k


class MinimumSpanningForest(_WeightedPatternApp):
    """Minimum spanning forest: gl_msf, Boruvka's algorithm over the rows with a weight per entry.  The matrix is
    read as an undirected weighted graph and stored in both directions by the host (io.symmetrize_weighted: the diagonal is
    dropped, every other stored entry is an edge -- a stored 0 included --, an edge stored more than once gets its smallest
    value, -0.0 becomes +0.0, NaN is refused; weighted=False: zero values are no edges and every weight is 1).  That matrix is
    kept as graph_, with the weights in adj_data; an all-ones copy of it is planned (the row copy would store a zero value as
    no entry).  Every result has one word per ENTRY of graph_, aligned with graph_.adj_indices.  Edges are ordered by (key(w),
    lo, hi), a strict total order, so the forest is unique: the one Kruskal's algorithm returns taking the edges in that order."""
    _no_shards_ = ("gl_msf reads the component of every column of a row and the rows of both ends of a chosen edge, so every rank "
                   "would need the whole symmetric matrix and the whole forest")
    in_forest_ = num_edges_ = num_components_ = labels_ = rounds_ = launches_ = None
    weighted_ = True

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True, weighted=True):
        self.weighted_ = bool(weighted)
        _PatternApp.load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows)

    def _prepare(self, csr):
        self.graph_, self.degrees_ = io.symmetrize_weighted(csr, self.weighted_)
        self.in_forest_ = None
        return self._ones_of_graph()

    def run(self, labels=False):
        """-> bool[graph_.nnz]: in_forest[j] = the edge of entry j is in the minimum spanning forest.  Leaves in_forest_, edges_
        (int64[m, 2]: (lo, hi) of every forest edge, ascending), weights_ (float32[m], aligned with edges_), total_weight_ (the
        f64 sum of weights_ in that order, added up on the host), num_edges_, num_components_ (over the n_real_ real vertices:
        padding vertices are singletons), labels_ (uint32[n_]: the smallest vertex of every vertex's component, or None without
        labels=True), rounds_ (Boruvka rounds in which a component chose an edge) and launches_.  The call waits for the
        device."""
        self._require_sent()
        B, n, nnz = self.backend, self.n_, self.graph_.nnz
        room = max(1, nnz)
        out = B.alloc(room + (n if labels else 0), np.float32)          # (32-bit words: the forest words, then the labels)
        stats = self.SpMV_.msf(self.weight_buf_, B.view(out, 0, room, 4), B.view(out, room, n, 4) if labels and n else None)
        B.sync()
        got = B.download(out, np.uint32, room + (n if labels else 0))
        self.in_forest_ = got[:nnz] != 0
        self.labels_ = got[room:] if labels else None
        self.num_edges_, components, self.rounds_, self.launches_ = stats
        self.num_components_ = components - (n - self.n_real_)
        self._collect_edges(lambda rows, cols: self.in_forest_)
        return self.in_forest_


class Matching(_WeightedPatternApp):
    """Greedy weighted matching: gl_match, the locally dominant matching over the rows with a weight per entry.
    The matrix is read as an undirected weighted graph and stored in both directions by the host (io.symmetrize_weighted with
    keep="largest": the diagonal is dropped, every other stored entry is an edge -- a stored 0 included --, an edge stored more
    than once gets its LARGEST value, -0.0 becomes +0.0, NaN is refused; weighted=False: KCore's reading, zero values are no
    edges and every weight is 1, which gives the lexicographically greedy maximal matching; drop_nonpositive=True removes the
    edges of weight <= 0 before planning, so that the half-approximation bound holds on signed data).  That matrix is kept as
    graph_, with the weights in adj_data; an all-ones copy of it is planned (the row copy would store a zero value as no
    entry).  Edges are ordered by (~key(w), lo, hi) -- heaviest first, then the smallest (lo, hi) --, a strict total order, so
    the result is unique: the matching that takes the edges greedily in that order."""
    _no_shards_ = ("gl_match reads the mate of every column of a row and the rows of both ends of a matched edge, so every rank "
                   "would need the whole symmetric matrix and every vertex's mate")
    mate_ = in_matching_ = num_matched_ = rounds_ = scans_ = launches_ = None
    weighted_, drop_nonpositive_ = True, False

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True, weighted=True, drop_nonpositive=False):
        self.weighted_, self.drop_nonpositive_ = bool(weighted), bool(drop_nonpositive)
        _PatternApp.load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows)

    def _prepare(self, csr):
        self.graph_, self.degrees_ = _matching_graph_of(csr, self.weighted_, self.drop_nonpositive_)
        self.mate_ = None
        return self._ones_of_graph()

    def run(self):
        """-> uint32[n_]: mate[v] = the vertex v is matched to, MATCH_FREE (0xffffffff) for a free vertex.  Leaves mate_,
        in_matching_ (bool[graph_.nnz]: the entry's edge is matched, both entries of an edge alike), edges_ (int64[m, 2]: (lo,
        hi) of every matched edge, ascending), weights_ (float32[m], aligned with edges_), total_weight_ (the f64 sum of
        weights_ in that order, added up on the host), num_matched_ (matched edges), rounds_ (rounds in which a vertex pointed
        or finished), scans_ (row scans of all rounds) and launches_.  The call waits for the device."""
        self._require_sent()
        B, n = self.backend, self.n_
        out = B.alloc(max(1, n), np.float32)                            # (32-bit words)
        stats = self.SpMV_.match(self.weight_buf_, out)
        B.sync()
        self.mate_ = B.download(out, np.uint32, max(1, n))[:n]
        self.num_matched_, self.rounds_, self.scans_, self.launches_ = stats
        self.in_matching_ = self._collect_edges(lambda rows, cols: self.mate_.astype(np.int64)[rows] == cols)
        return self.mate_


class GraphColoring(_PatternApp):
    """Graph colouring: gl_color, Jones-Plassmann colouring with dependency counters.  The matrix is read as an
    undirected simple graph -- duplicates, the diagonal, zero-valued entries and direction are ignored, as in KCore -- and stored
    in both directions by the host (io.symmetrize_simple): colouring v must reach every neighbour of v through row v.  The result
    is the sequential first-fit greedy colouring in the order the priorities give, to the bit."""
    _no_shards_ = "gl_color reads row u for every column u of a row, so every rank would need the whole symmetric matrix"
    degrees_ = colors_ = priorities_ = num_colors_ = rounds_ = launches_ = widest_ = degeneracy_ = color_sizes_ = None

    def _prepare(self, csr):
        csr, self.degrees_ = io.symmetrize_simple(csr)
        return csr

    def run(self, order="largest_first", seed=0, priorities=None):
        """-> uint32[n_]: colors[v] = the smallest colour that no neighbour going before v has (padding vertices: 0).  The order
        is io.coloring_priorities(degrees_, order, seed) -- "natural", "random", "largest_first" or "smallest_last", which first
        runs gl_kcore on the same plan for its peeling order and then needs at most degeneracy_ + 1 colours -- or an explicit
        `priorities` array of n_real_ or n_ words (larger first, ties to the smaller vertex number), which overrides `order`.
        Leaves colors_, priorities_ (uint32[n_], the array the run used; None for natural), num_colors_, rounds_ (the depth of
        the order's DAG), launches_, widest_ (the most vertices coloured by one round, padding vertices included), degeneracy_
        (None unless "smallest_last" ran) and color_sizes_[c] = real vertices of colour c.  The call waits for the device."""
        self._require_sent()
        B, n = self.backend, self.n_
        self.degeneracy_ = None
        if priorities is not None:
            prio = np.asarray(priorities)
            if prio.ndim != 1 or prio.shape[0] not in (self.n_real_, n):
                raise ValueError("GraphColoring.run(): priorities of shape %s, expected %d or %d words" % (prio.shape, self.n_real_, n))
            prio = np.concatenate([prio.astype(np.uint32), np.zeros(n - prio.shape[0], dtype=np.uint32)])
        elif order == "smallest_last":
            peel_order, self.degeneracy_ = self._peel_order()
            prio = io.coloring_priorities(self.degrees_, order, seed, peel_order=peel_order)
        else:
            prio = io.coloring_priorities(self.degrees_, order, seed)
        out = B.alloc(2 * n if prio is not None else n, np.float32)  # (32-bit words: the colours, then the priorities)
        if prio is not None:
            B.upload(B.view(out, n, n, 4), prio)
        stats = self.SpMV_.color(B.view(out, 0, n, 4), B.view(out, n, n, 4) if prio is not None else None)
        B.sync()
        self.colors_ = B.download(out, np.uint32, n)
        self.priorities_ = prio
        self.num_colors_, self.rounds_, self.launches_, self.widest_ = stats
        self.color_sizes_ = np.bincount(self.colors_[:self.n_real_], minlength=self.num_colors_).astype(np.int64)
        return self.colors_

    def independent_set(self, c=0):
        """-> bool[n_]: the vertices of colour c of the last run -- an independent set; padding vertices are in none.  Class 0 is
        a MAXIMAL independent set, the first-fit one of the run's order: every other vertex has a neighbour in it."""
        if self.colors_ is None:
            raise RuntimeError("GraphColoring.independent_set(): run() first")
        mask = self.colors_ == c
        mask[self.n_real_:] = False
        return mask


class LabelPropagation(_PatternApp):
    """Label propagation communities: gl_lpa, Raghavan, Albert & Kumara's rule swept colour class by colour
    class (Cordasco & Gargano).  The matrix is read as an undirected simple graph -- duplicates, the diagonal, zero-valued
    entries and direction are ignored, as in KCore and GraphColoring -- and stored in both directions by the host
    (io.symmetrize_simple).  Evaluating a vertex gives it the smallest of its neighbours' most frequent labels if strictly more
    neighbours carry that label than its own; under a proper colouring the sweeps equal the sequential loop in (colour, vertex)
    order, reach a fixed point, and the result is a pure function of (graph, colouring, initial labels), to the bit."""
    _no_shards_ = ("gl_lpa reads the label of every column of a row and flags the rows of a changed vertex's neighbours, so every "
                   "rank would need the whole symmetric matrix and every vertex's label")
    degrees_ = graph_ = labels_ = colors_ = initial_ = num_colors_ = sweeps_ = changes_ = evaluations_ = launches_ = converged_ = None
    num_communities_ = community_labels_ = community_sizes_ = None

    def _prepare(self, csr):
        self.graph_, self.degrees_ = io.symmetrize_simple(csr)
        self.labels_ = None
        return self.graph_

    def run(self, max_sweeps=100, initial=None, seed=None, order="largest_first", colors=None, synchronous=False):
        """-> uint32[n_]: labels[v] = the community label of v (padding vertices are isolated and keep their own numbers).
        The sweeps go colour class by colour class under `colors` (n_real_ or n_ words, a proper colouring) or, without them,
        under the colouring SpMV_.color gives on the same plan for io.coloring_priorities(degrees_, order, seed or 0)
        ("smallest_last" first runs gl_kcore, as GraphColoring does); synchronous=True sweeps all vertices at once from the
        previous sweep's labels instead, which may oscillate until max_sweeps.  `initial` (n_real_ or n_ words, none
        0xffffffff) are the labels the vertices start with -- seed labels, or a relabelling that undoes the pull towards small
        vertex numbers that the rule's tie-break has; without it, `seed` gives io.lpa_initial_labels(n_real_, seed), a random
        permutation, and seed=None every vertex's own number.  Leaves labels_, colors_ (uint32[n_]; None when synchronous),
        num_colors_ (classes swept), initial_ (the array the run used; None for own numbers), sweeps_, changes_,
        evaluations_, launches_ (gl_lpa's alone), converged_, and over the real vertices num_communities_,
        community_labels_ (ascending) and community_sizes_ (aligned with them).  The call waits for the device."""
        self._require_sent()
        B, n = self.backend, self.n_
        out = B.alloc(3 * max(1, n), np.float32)                     # (32-bit words: the labels, the colours, the priorities / initial labels)
        label_buf, color_buf, third = B.view(out, 0, n, 4), B.view(out, n, n, 4), B.view(out, 2 * n, n, 4)

        def padded(arr, what, fill):
            a = np.asarray(arr)
            if a.ndim != 1 or a.shape[0] not in (self.n_real_, n):
                raise ValueError("LabelPropagation.run(): %s of shape %s, expected %d or %d words" % (what, a.shape, self.n_real_, n))
            return np.concatenate([a.astype(np.uint32), fill[a.shape[0]:]])

        own = np.arange(n, dtype=np.uint32)
        if initial is not None:
            start = padded(initial, "initial", own)
        else:
            start = io.lpa_initial_labels(self.n_real_, seed, n) if seed is not None else None
        if synchronous:
            self.colors_, self.num_colors_ = None, 1
        elif colors is not None:
            self.colors_ = padded(colors, "colors", np.zeros(n, dtype=np.uint32))
            self.num_colors_ = int(self.colors_.max()) + 1 if n else 0
            B.upload(color_buf, self.colors_)
        else:
            seed0 = 0 if seed is None else seed
            if order == "smallest_last":
                prio = io.coloring_priorities(self.degrees_, order, seed0, peel_order=self._peel_order()[0])
            else:
                prio = io.coloring_priorities(self.degrees_, order, seed0)
            if prio is not None:
                B.upload(third, prio)
            self.num_colors_ = self.SpMV_.color(color_buf, third if prio is not None else None)[0]
            B.sync()
            self.colors_ = B.download(out, np.uint32, 2 * n)[n:]
        if start is not None:
            B.upload(third, start)
        stats = self.SpMV_.lpa(label_buf, None if synchronous else color_buf, third if start is not None else None, max_sweeps)
        B.sync()
        self.labels_ = B.download(out, np.uint32, n)
        self.initial_ = start
        self.sweeps_, self.changes_, self.evaluations_, self.launches_, self.converged_ = stats
        self.community_labels_, sizes = np.unique(self.labels_[:self.n_real_], return_counts=True)
        self.community_sizes_ = sizes.astype(np.int64)
        self.num_communities_ = int(sizes.shape[0])
        return self.labels_

    def modularity(self, labels=None):
        """-> float: Newman's modularity sum_c e_c / m - (d_c / 2 m)^2 of the last run's labels (or of `labels`, n_ words) on
        graph_, computed on the host in f64: e_c = edges inside community c, d_c = the degrees of its vertices, m = edges
        (0.0 for a graph without edges)"""
        lab = self.labels_ if labels is None else np.asarray(labels)
        if lab is None:
            raise RuntimeError("LabelPropagation.modularity(): run() first")
        return _modularity_of(self.graph_, self.degrees_, lab)


class Louvain(_PatternApp):
    """Louvain communities: gl_louvain_move, Blondel et al.'s modularity optimisation with the local moving
    swept colour class by colour class (Lu, Halappanavar & Kalyanaraman).  The matrix is read as an undirected simple graph --
    duplicates, the diagonal, zero-valued entries and direction are ignored, as in LabelPropagation -- and stored in both
    directions by the host (io.symmetrize_simple); input edge weights are not read: level 0 has every weight 1 and k = the
    degrees.  Every level moves vertices on the device until a sweep gains no more than tol, then the host aggregates the
    communities into the next level's weighted graph (io.aggregate_communities).  Integer arithmetic throughout: the result is
    a pure function of (graph, colourings, tol, max_sweeps, max_levels), to the bit."""
    _no_shards_ = ("gl_louvain_move reads the label of every column of a row and the total of every neighbouring community, so "
                   "every rank would need every label and the whole tot array")
    degrees_ = graph_ = labels_ = levels_ = level_sizes_ = level_colors_ = level_sweeps_ = level_moves_ = level_q_ = launches_ = None
    num_communities_ = community_labels_ = community_sizes_ = dendrogram_ = level_colorings_ = timings_ = None

    def _prepare(self, csr):
        self.graph_, self.degrees_ = io.symmetrize_simple(csr)
        self.labels_ = None
        return self.graph_

    def run(self, tol=1e-7, max_sweeps=100, max_levels=32, order="largest_first", seed=0):
        """-> uint32[n_]: labels[v] = the SMALLEST original vertex of v's community (ConnectedComponents' convention; isolated
        and padding vertices keep their own numbers).  Level 0 runs on this driver's own module, every later level on a fresh
        SpMVModule plan of the aggregated pattern; each level is coloured by SpMV.color under io.coloring_priorities(that
        level's pattern degrees, order, seed) ("smallest_last" first runs gl_kcore on the level's plan) and moved by
        gl_louvain_move with min_gain = floor(tol * two_m^2).  A level is ACCEPTED iff it moved something and its q_last is
        strictly above the last accepted Q (at the start: the singletons' Q); otherwise it is discarded and the run ends, as it
        does when a level merges nothing or max_levels is reached.  Leaves labels_, levels_ (accepted levels), and per level
        RUN (a discarded last one included) level_sizes_ (vertices), level_colors_ (classes), level_sweeps_, level_moves_,
        level_q_ (int64[runs, 2]: q_first and q_last, modularity x two_m^2), level_colorings_ (the colourings used);
        launches_ (gl_louvain_move's alone), dendrogram_ (per accepted level, uint32[n_]: the community of every original
        vertex), num_communities_, community_labels_ (ascending) and community_sizes_ over the real vertices, and timings_
        (seconds: color, move, aggregate, plan).  The call waits for the device."""
        self._require_sent()
        B = self.backend
        clock = {"color": 0.0, "move": 0.0, "aggregate": 0.0, "plan": 0.0}
        live = {}

        def module_of(level, graph):
            if level == 0:
                return self.SpMV_, graph.num_rows
            if live.get("level") != level:
                t0 = time.perf_counter()
                padded = graph.copy()
                self._pad(padded)
                mod = self.backend.SpMVModule(self.num_channels_, 0, 0)
                mod.set_semiring(self.semiring_)
                mod.set_mask_type(M.kNoMask)
                mod.load_and_format_matrix(padded, True)
                mod.send_matrix_host_to_device()
                live.update(level=level, module=mod, rows=padded.num_rows)
                clock["plan"] += time.perf_counter() - t0
            return live["module"], live["rows"]

        def color(level, graph, deg):
            mod, rows = module_of(level, graph)
            t0 = time.perf_counter()
            deg = np.concatenate([deg, np.zeros(rows - deg.shape[0], dtype=np.uint32)])
            buf = B.alloc(2 * max(1, rows), np.float32)                 # (32-bit words: the colours, then the priorities)
            if order == "smallest_last":
                peel = B.alloc(2 * max(1, rows), np.float32)
                mod.kcore(B.view(peel, 0, rows, 4), B.view(peel, rows, rows, 4))
                B.sync()
                prio = io.coloring_priorities(deg, order, seed, peel_order=B.download(peel, np.uint32, 2 * rows)[rows:])
            else:
                prio = io.coloring_priorities(deg, order, seed)
            if prio is not None:
                B.upload(B.view(buf, rows, rows, 4), prio)
            num_colors = mod.color(B.view(buf, 0, rows, 4), B.view(buf, rows, rows, 4) if prio is not None else None)[0]
            B.sync()
            colors = B.download(buf, np.uint32, rows)
            live["color_buf"] = buf
            clock["color"] += time.perf_counter() - t0
            return colors, num_colors

        def move(level, graph, weights, k, colors, min_gain):
            mod, rows = module_of(level, graph)
            t0 = time.perf_counter()
            nnz = graph.nnz
            buf = B.alloc(2 * max(1, rows) + max(1, nnz), np.float32)   # (32-bit words: the labels, k, the entry weights)
            label_buf, k_buf, w_buf = B.view(buf, 0, rows, 4), B.view(buf, rows, rows, 4), B.view(buf, 2 * rows, nnz, 4)
            if level:
                B.upload(k_buf, np.concatenate([k, np.zeros(rows - k.shape[0], dtype=np.uint32)]))
                if nnz:
                    B.upload(w_buf, weights)
            stats = mod.louvain_move(label_buf, B.view(live["color_buf"], 0, rows, 4), w_buf if level and nnz else None,
                                     k_buf if level else None, max_sweeps, min_gain)
            B.sync()
            labels = B.download(buf, np.uint32, rows)
            clock["move"] += time.perf_counter() - t0
            return (labels,) + tuple(stats)

        t_all = time.perf_counter()
        res = _louvain_levels(self.graph_, self.degrees_, move, color, tol, max_sweeps, max_levels)
        clock["aggregate"] = time.perf_counter() - t_all - clock["color"] - clock["move"] - clock["plan"]
        live.clear()
        self.labels_ = res["labels"]
        self.levels_ = res["levels"]
        self.level_sizes_ = np.asarray(res["sizes"], dtype=np.int64)
        self.level_colors_ = np.asarray(res["colors"], dtype=np.int64)
        self.level_sweeps_ = np.asarray(res["sweeps"], dtype=np.int64)
        self.level_moves_ = np.asarray(res["moves"], dtype=np.int64)
        self.level_q_ = np.asarray(res["q"], dtype=np.int64).reshape(-1, 2)
        self.level_colorings_ = res["colorings"]
        self.launches_ = res["launches"]
        self.dendrogram_ = res["dendrogram"]
        self.timings_ = clock
        self.community_labels_, sizes = np.unique(self.labels_[:self.n_real_], return_counts=True)
        self.community_sizes_ = sizes.astype(np.int64)
        self.num_communities_ = int(sizes.shape[0])
        return self.labels_

    def modularity(self, labels=None):
        """-> float: Newman's modularity of the last run's labels (or of `labels`, n_ words) on graph_, on the host in f64
        (_modularity_of, LabelPropagation.modularity's formula)"""
        lab = self.labels_ if labels is None else np.asarray(labels)
        if lab is None:
            raise RuntimeError("Louvain.modularity(): run() first")
        return _modularity_of(self.graph_, self.degrees_, lab)


class StronglyConnectedComponents(_PatternApp):
    """Strongly connected components: gl_scc, trimming and colour-and-collect passes over the pattern and its
    transpose.  The matrix is read as a simple DIRECTED graph (io.simple_pattern: an edge u -> v for a stored non-zero A[v, u], u
    != v; zero values, the diagonal and duplicates dropped, rows ascending); the transposed pattern lives in a second boolean
    SpMVModule, out_, which exists only when the pattern is not symmetric.  run() labels every vertex with the smallest vertex
    of its component, ConnectedComponents' convention: on a symmetric pattern the two agree to the bit."""
    _no_shards_ = ("gl_scc reads the colour of every column of a row, in the pattern and in its transpose, so every rank would need "
                   "both whole patterns")
    ORDERS = ("natural", "random", "largest_first")
    graph_ = graph_out_ = symmetric_ = degrees_ = labels_ = priorities_ = num_components_ = largest_component_ = None
    component_labels_ = component_sizes_ = trimmed_ = passes_ = rounds_ = launches_ = is_dag_ = None

    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, vec_buf_len=0, comm=None, backend=None):
        _PatternApp.__init__(self, num_channels, spmv_out_buf_len, vec_buf_len, comm, backend)
        self.buf_lens_ = (spmv_out_buf_len, vec_buf_len)
        self.out_ = None                 # the transposed pattern's module (a pattern that is not symmetric)

    def _prepare(self, csr):
        self.graph_, self.graph_out_, self.symmetric_ = io.simple_pattern(csr)      # (after padding: padding vertices have empty rows)
        n = self.graph_.num_rows
        self.degrees_ = (np.diff(self.graph_.adj_indptr.astype(np.int64))
                         + np.bincount(self.graph_.adj_indices, minlength=n)).astype(np.uint32)      # in-degree + out-degree
        self.labels_ = None
        return self.graph_

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True):
        _PatternApp.load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows)
        self.modules_ = [self.SpMV_]
        self.out_ = None
        if not self.symmetric_:
            self.out_ = self.backend.SpMVModule(self.num_channels_, *self.buf_lens_)
            self.out_.set_semiring(M.LogicalSemiring)
            self.out_.set_mask_type(M.kNoMask)
            self.out_.blocking = False
            self.out_.load_and_format_matrix(self.graph_out_, skip_empty_rows)
            self.add_module(self.out_)

    def send_matrix_host_to_device(self):
        _PatternApp.send_matrix_host_to_device(self)
        if self.out_ is not None:
            self.out_.send_matrix_host_to_device()

    def run(self, order="largest_first", seed=0, priorities=None):
        """-> uint32[n_]: labels[v] = the smallest vertex u such that v reaches u and u reaches v (padding vertices are
        singletons).  The priorities decide which component every pass removes -- its best-keyed live vertex's, larger priority
        first, ties to the smaller vertex -- and never the labels: io.coloring_priorities(degrees_, order, seed) for "natural",
        "random" or "largest_first" (degrees_ = in-degree + out-degree: hubs first normally collects the giant component in
        pass 1), or an explicit `priorities` array of n_real_ or n_ words, which overrides `order`.  Leaves labels_, priorities_
        (uint32[n_], the array the run used; None for natural), trimmed_, passes_, rounds_, launches_ and, over the n_real_ real
        vertices, num_components_, largest_component_, component_labels_ (ascending), component_sizes_ (aligned with them) and
        is_dag_ (every component is a single vertex).  The call waits for the device."""
        self._require_sent()
        B, n = self.backend, self.n_
        if priorities is not None:
            prio = np.asarray(priorities)
            if prio.ndim != 1 or prio.shape[0] not in (self.n_real_, n):
                raise ValueError("StronglyConnectedComponents.run(): priorities of shape %s, expected %d or %d words"
                                 % (prio.shape, self.n_real_, n))
            prio = np.concatenate([prio.astype(np.uint32), np.zeros(n - prio.shape[0], dtype=np.uint32)])
        elif order in self.ORDERS:
            prio = io.coloring_priorities(self.degrees_, order, seed)
        else:
            raise ValueError("StronglyConnectedComponents.run(): order %r is none of %s" % (order, ", ".join(self.ORDERS)))
        out = B.alloc(2 * n if prio is not None else n, np.float32)  # (32-bit words: the labels, then the priorities)
        if prio is not None:
            B.upload(B.view(out, n, n, 4), prio)
        stats = self.SpMV_.scc(self.out_, B.view(out, 0, n, 4), B.view(out, n, n, 4) if prio is not None else None)
        B.sync()
        self.labels_ = B.download(out, np.uint32, n)
        self.priorities_ = prio
        components, self.passes_, self.trimmed_, self.rounds_, self.launches_ = stats
        if self.graph_.nnz:
            self.trimmed_ -= n - self.n_real_                        # (every padding vertex was trimmed; without entries nothing runs)
        self.num_components_ = components - (n - self.n_real_)
        self.component_labels_, sizes = np.unique(self.labels_[:self.n_real_], return_counts=True)
        self.component_sizes_ = sizes.astype(np.int64)
        self.largest_component_ = int(sizes.max()) if sizes.size else 0
        self.is_dag_ = self.largest_component_ <= 1
        return self.labels_

    def condensation(self):
        """-> (CSRMatrix, rank_of_label): the graph between the components of the last run, on the host (numpy).  The
        components of the real vertices are ranked by ascending label, rank_of_label[l] = the rank of the component labelled l
        (uint32[n_real_], 0xffffffff where l is no label); the matrix is num_components_ x num_components_ and, as everywhere
        here, an entry A[b, a] = 1 is an edge a -> b: some u in component a has an edge to some v in component b != a.  It is
        the simple pattern of a DAG: rows ascending, no diagonal, no duplicates."""
        if self.labels_ is None:
            raise RuntimeError("StronglyConnectedComponents.condensation(): run() first")
        nr, k = self.n_real_, int(self.num_components_)
        rank = np.full(nr, 0xFFFFFFFF, dtype=np.uint32)
        rank[self.component_labels_.astype(np.int64)] = np.arange(k, dtype=np.uint32)
        src, dst = _edges_of_pattern(self.graph_, nr)
        lab = self.labels_.astype(np.int64)
        a, b = rank[lab[src]].astype(np.int64), rank[lab[dst]].astype(np.int64)
        key = np.unique(b[a != b] * k + a[a != b])
        indptr = np.zeros(k + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // max(k, 1), minlength=k), out=indptr[1:])
        dag = io.CSRMatrix(k, k, np.ones(key.shape[0], dtype=np.float32), (key % max(k, 1)).astype(np.uint32), indptr.astype(np.uint32))
        return dag, rank


class BiconnectedComponents(_PatternApp):
    """Biconnected components: gl_bicc, Tarjan and Vishkin's algorithm over a deterministic BFS forest.  The
    matrix is read as an undirected simple graph -- duplicates, the diagonal, zero-valued entries and direction are ignored, as in
    KTruss -- and stored in both directions by the host (io.symmetrize_simple); that matrix is kept as graph_, and the block labels
    have one word per ENTRY of it, aligned with graph_.adj_indices: both entries of an edge carry the same value."""
    _no_shards_ = ("gl_bicc reads the level, the parent and the preorder number of every column of a row, so every rank would need "
                   "the whole symmetric matrix")
    degrees_ = graph_ = block_ = vertex_blocks_ = articulation_ = bridge_ = edge_component_ = None
    num_blocks_ = num_articulation_ = num_bridges_ = num_trees_ = depth_ = launches_ = None
    block_labels_ = block_sizes_ = largest_block_ = None

    def _prepare(self, csr):
        csr, self.degrees_ = io.symmetrize_simple(csr)
        self.graph_ = csr
        self.block_ = None
        return csr

    def run(self, edge_components=False):
        """-> uint32[graph_.nnz]: block[j] = the smallest entry number of the block (biconnected component) that holds the edge of
        entry j.  Leaves block_, vertex_blocks_ (uint32[n_]: the blocks a vertex belongs to; padding vertices are isolated: 0),
        articulation_ (bool[n_]: two blocks or more), bridge_ (bool per entry: its block has two entries), edge_component_
        (uint32[n_], the smallest vertex of every vertex's 2-edge-connected component, or None without edge_components=True),
        num_blocks_, num_articulation_, num_bridges_, num_trees_ (over the real vertices), depth_ (the largest level of the BFS
        forest), launches_, block_labels_ (ascending), block_sizes_ (edges per block, aligned with them) and largest_block_.  The
        device's bridge and articulation counts must equal the ones derived from block_ and vertex_blocks_.  The call waits
        for the device."""
        self._require_sent()
        B, n, nnz = self.backend, self.n_, self.graph_.nnz
        room = max(1, nnz)
        out = B.alloc(room + (2 * n if edge_components else n), np.float32)    # (32-bit words: block, vertex_blocks, edge_component)
        stats = self.SpMV_.bicc(B.view(out, 0, room, 4), B.view(out, room, n, 4), B.view(out, room + n, n, 4) if edge_components else None)
        B.sync()
        got = B.download(out, np.uint32, room + (2 * n if edge_components else n))
        self.block_ = got[:nnz]
        self.vertex_blocks_ = got[room:room + n]
        self.edge_component_ = got[room + n:] if edge_components else None
        self.num_blocks_, self.num_articulation_, self.num_bridges_, self.depth_, self.launches_, trees = stats
        self.num_trees_ = trees - (n - self.n_real_)
        self.articulation_ = self.vertex_blocks_ >= 2
        self.block_labels_, entries = np.unique(self.block_, return_counts=True)
        self.block_sizes_ = (entries // 2).astype(np.int64)
        self.largest_block_ = int(self.block_sizes_.max()) if entries.size else 0
        per_label = np.zeros(room, dtype=np.int64)
        per_label[self.block_labels_.astype(np.int64)] = entries
        self.bridge_ = per_label[self.block_.astype(np.int64)] == 2
        assert self.num_blocks_ == self.block_labels_.shape[0], (self.num_blocks_, self.block_labels_.shape[0])
        assert self.num_bridges_ == int(np.count_nonzero(entries == 2)), (self.num_bridges_, int(np.count_nonzero(entries == 2)))
        assert self.num_articulation_ == int(np.count_nonzero(self.articulation_)), (self.num_articulation_, int(np.count_nonzero(self.articulation_)))
        return self.block_

    def block_cut_tree(self):
        """-> (CSRMatrix, block_rank, cut_rank): the forest between the blocks and the articulation points of the last run, on the
        host (numpy) -- the counterpart of StronglyConnectedComponents.condensation().  The blocks are ranked by ascending label,
        block_rank[l] = the rank of the block labelled l (uint32[graph_.nnz], 0xffffffff where l is no label): nodes 0 ..
        num_blocks_ - 1; the articulation points follow in ascending vertex order, cut_rank[v] = the node of vertex v
        (uint32[n_], 0xffffffff where v is none).  The matrix is symmetric and bipartite: an entry between a block and an
        articulation point that belongs to it; rows ascending.  It is a forest: one tree per component with an edge."""
        if self.block_ is None:
            raise RuntimeError("BiconnectedComponents.block_cut_tree(): run() first")
        n, nnz, k = self.n_, self.graph_.nnz, int(self.num_blocks_)
        block_rank = np.full(nnz, 0xFFFFFFFF, dtype=np.uint32)
        block_rank[self.block_labels_.astype(np.int64)] = np.arange(k, dtype=np.uint32)
        cuts = np.flatnonzero(self.articulation_)
        cut_rank = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        cut_rank[cuts] = k + np.arange(cuts.shape[0], dtype=np.uint32)
        nodes = k + cuts.shape[0]
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.graph_.adj_indptr.astype(np.int64)))
        at = self.articulation_[rows]
        a, b = cut_rank[rows[at]].astype(np.int64), block_rank[self.block_.astype(np.int64)[at]].astype(np.int64)
        key = np.unique(np.concatenate([a * max(nodes, 1) + b, b * max(nodes, 1) + a]))
        indptr = np.zeros(nodes + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // max(nodes, 1), minlength=nodes), out=indptr[1:])
        tree = io.CSRMatrix(nodes, nodes, np.ones(key.shape[0], dtype=np.float32), (key % max(nodes, 1)).astype(np.uint32), indptr.astype(np.uint32))
        return tree, block_rank, cut_rank


class TopologicalOrder(_PatternApp):
    """Topological levels, a topological order and the critical path: gl_topo, Kahn's peeling with dependency
    counters over the pattern and its transpose.  The matrix is read as a DIRECTED graph (io.directed_weighted: an edge u -> v for
    a stored entry A[v, u], u != v; weighted=False is io.simple_pattern's reading, weighted=True keeps every stored entry with the
    largest of its values, -0.0 as +0.0, NaN and inf refused); the transposed pattern lives in a second boolean SpMVModule, out_,
    which exists only when the pattern is not symmetric.  Both plans are built from ones (the row copy would store a zero value
    as no entry); the weights travel in buffers of their own, aligned with graph_.adj_indices and graph_out_.adj_indices.
    load_and_format_matrix accepts a path or a CSRMatrix, so StronglyConnectedComponents.condensation()'s matrix goes straight in.
    On a cyclic input the peeled vertices are those that are neither on a cycle nor behind one."""
    _no_shards_ = ("gl_topo decrements the counter of every column of a row of the transposed pattern and reads the distance of "
                   "every column of a row of the pattern, so every rank would need both whole patterns and every counter")
    graph_ = graph_out_ = symmetric_ = weight_buf_ = weight_out_buf_ = None
    level_ = is_dag_ = num_peeled_ = cyclic_ = num_levels_ = level_sizes_ = widest_ = launches_ = None
    dist_ = parent_ = critical_length_ = order_ = position_ = None
    weighted_ = False

    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, vec_buf_len=0, comm=None, backend=None):
        _PatternApp.__init__(self, num_channels, spmv_out_buf_len, vec_buf_len, comm, backend)
        self.buf_lens_ = (spmv_out_buf_len, vec_buf_len)
        self.out_ = None                 # the transposed pattern's module (a pattern that is not symmetric)

    @staticmethod
    def _ones_of(g):
        return io.CSRMatrix(g.num_rows, g.num_cols, np.ones(g.nnz, dtype=np.float32), g.adj_indices, g.adj_indptr)

    def _prepare(self, csr):
        self.graph_, self.graph_out_, self.symmetric_ = io.directed_weighted(csr, self.weighted_)      # (after padding)
        self.level_ = self.dist_ = self.parent_ = self.order_ = self.position_ = None
        self.weight_buf_ = self.weight_out_buf_ = None
        return self._ones_of(self.graph_)

    def load_and_format_matrix(self, src, skip_empty_rows=True, weighted=False):
        self.weighted_ = bool(weighted)
        _PatternApp.load_and_format_matrix(self, src, skip_empty_rows)
        self.modules_ = [self.SpMV_]
        self.out_ = None
        if not self.symmetric_:
            self.out_ = self.backend.SpMVModule(self.num_channels_, *self.buf_lens_)
            self.out_.set_semiring(M.LogicalSemiring)
            self.out_.set_mask_type(M.kNoMask)
            self.out_.blocking = False
            self.out_.load_and_format_matrix(self._ones_of(self.graph_out_), skip_empty_rows)
            self.add_module(self.out_)

    def send_matrix_host_to_device(self):
        _PatternApp.send_matrix_host_to_device(self)
        if self.out_ is not None:
            self.out_.send_matrix_host_to_device()
        if self.weighted_:
            for name, g in (("weight_buf_", self.graph_), ("weight_out_buf_", self.graph_out_)):
                buf = self.backend.alloc(max(1, g.nnz), np.float32)
                if g.nnz:
                    self.backend.upload(buf, g.adj_data)
                setattr(self, name, buf)

    def run(self, reverse=False, order=False):
        """-> uint32[n_]: level[v] = the edges of the longest path that ends in v, 0xffffffff for a vertex on a cycle or behind
        one (padding vertices are isolated: level 0).  reverse=True swaps the two plans: HEIGHTS, the longest path that starts
        in v, and (weighted) the distance to a sink with the successor tree.  Leaves level_, launches_ and, over the n_real_
        real vertices, num_peeled_, is_dag_, cyclic_ (bool[n_real_]: not peeled), level_sizes_ (int64: the vertices of every
        level), num_levels_ and widest_; on a weighted load also dist_ (float32[n_]: bits 0x7fc00000 when unpeeled), parent_
        (uint32[n_]: the smallest neighbour that attains dist_, 0xffffffff on sources and unpeeled vertices) and
        critical_length_ (the largest dist_ of a peeled real vertex; None when nothing is peeled); with order=True order_ (the
        peeled real vertices sorted by (level, vertex): a topological order, canonicalised on the host from the device's queue)
        and position_ (uint32[n_real_]: where a vertex stands in order_, 0xffffffff when unpeeled).  The call waits for the
        device."""
        self._require_sent()
        B, n, nr = self.backend, self.n_, self.n_real_
        pin, pout, wbuf = self.SpMV_, self.out_, self.weight_buf_
        if reverse:
            wbuf = self.weight_out_buf_
            if self.out_ is not None:
                pin, pout = self.out_, self.SpMV_
        room = max(1, n)
        out = B.alloc(4 * room, np.float32)                          # (32-bit words: level, queue, dist, parent)
        w = self.weighted_
        stats = pin.topo(pout, B.view(out, 0, room, 4), B.view(out, room, room, 4) if order else None, wbuf if w else None,
                         B.view(out, 2 * room, room, 4) if w else None, B.view(out, 3 * room, room, 4) if w else None)
        B.sync()
        got = B.download(out, np.uint32, 4 * room)
        self.level_ = got[:n].copy()
        peeled = self.level_[:nr] != 0xFFFFFFFF
        self.cyclic_ = ~peeled
        self.num_peeled_ = int(np.count_nonzero(peeled))
        self.is_dag_ = self.num_peeled_ == nr
        self.level_sizes_ = np.bincount(self.level_[:nr][peeled].astype(np.int64)).astype(np.int64)
        self.num_levels_ = int(self.level_sizes_.shape[0])
        self.widest_ = int(self.level_sizes_.max()) if self.num_levels_ else 0
        self.launches_ = stats[3]
        assert stats[0] == self.num_peeled_ + (n - nr), "gl_topo's count of peeled vertices and its levels disagree"
        self.dist_ = self.parent_ = self.critical_length_ = None
        if w:
            self.dist_ = got[2 * room:2 * room + n].copy().view(np.float32)
            self.parent_ = got[3 * room:3 * room + n].copy()
            if self.num_peeled_:
                self.critical_length_ = float(self.dist_[:nr][peeled].max())
        self.order_ = self.position_ = None
        if order:
            queue = got[room:room + int(stats[0])].astype(np.int64)
            queue = queue[queue < nr]
            self.order_ = queue[np.lexsort((queue, self.level_[queue]))].astype(np.uint32)
            self.position_ = np.full(nr, 0xFFFFFFFF, dtype=np.uint32)
            self.position_[self.order_.astype(np.int64)] = np.arange(self.order_.shape[0], dtype=np.uint32)
        return self.level_

    def critical_path(self):
        """-> int64[k]: the vertices of a longest weighted path of the last run, from the smallest real vertex of largest dist_
        back along parent_ to a vertex without one (reverse=False: the path's END comes first; reverse=True: its start)."""
        if self.dist_ is None:
            raise RuntimeError("TopologicalOrder.critical_path(): run() on a weighted load first")
        if not self.num_peeled_:
            return np.zeros(0, dtype=np.int64)
        nr = self.n_real_
        peeled = ~self.cyclic_
        v = int(np.flatnonzero(peeled & (self.dist_[:nr] == np.float32(self.critical_length_)))[0])
        path = [v]
        while self.parent_[path[-1]] != 0xFFFFFFFF:
            path.append(int(self.parent_[path[-1]]))
        return np.asarray(path, dtype=np.int64)


class BetweennessCentrality(_PatternApp):
    """Betweenness centrality (an extension: the reference has no such driver): Brandes' algorithm, one search per source.  The
    search is an app.BFS this object owns, loaded with the simple pattern of the matrix (io.simple_pattern: zero values, the
    diagonal and duplicates dropped, rows ascending); its levels stay on the device, and gl_bc_accumulate
    counts the shortest paths level by level through that BFS's SpMV plan and adds every vertex's dependency, pulled through
    the transposed pattern's plan -- a second boolean SpMVModule, which exists only when the pattern is not symmetric."""

    _no_shards_ = ("gl_bc_accumulate reads the level and the path count of every column of a row, so every rank would need both "
                   "whole matrices")

    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, spmspv_out_buf_len=0, vec_buf_len=0, comm=None,
                 backend=None):
        _GraphApp.__init__(self, num_channels, comm, backend)
        self._refuse_shards()
        self.buf_lens_ = (spmv_out_buf_len, vec_buf_len)
        self.bfs_ = BFS(num_channels, spmv_out_buf_len, spmspv_out_buf_len, vec_buf_len, backend=self.backend)
        self.SpMV_ = self.bfs_.SpMV_
        self.out_ = None                 # the transposed pattern's module (a pattern that is not symmetric, or directed=True)
        for m in self.bfs_.modules_:
            self.add_module(m)
        self.sent_ = self.empty_ = False
        self.directed_ = None
        self.bc_ = self.sources_ = self.depths_ = self.reached_ = self.orphans_ = self.overflowed_ = None

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True, directed=None):
        """directed=None: undirected iff the pattern is symmetric; False on an asymmetric pattern takes every edge in both
        directions (io.symmetrize_simple); True keeps two plans even when the pattern is symmetric."""
        csr = self._load(csr_float_npz_path)
        n_real = csr.num_rows
        self._pad(csr)
        cin, cout, self.directed_ = _bc_patterns(csr, directed)      # (after padding: padding vertices have empty rows)
        self.n_, self.n_real_ = cin.num_rows, n_real
        self.empty_ = cin.nnz == 0                                  # an empty graph: nothing is loaded, run() launches nothing
        self.out_ = None
        self.modules_ = list(self.bfs_.modules_)
        if not self.empty_:
            self.bfs_.load_and_format_matrix(cin, skip_empty_rows)
            assert self.bfs_.n_ == self.n_
            if cout is not None:
                self.out_ = self.backend.SpMVModule(self.num_channels_, *self.buf_lens_)
                self.out_.set_semiring(M.LogicalSemiring)
                self.out_.set_mask_type(M.kNoMask)
                self.out_.blocking = False
                self.out_.load_and_format_matrix(cout, skip_empty_rows)
                self.add_module(self.out_)
        self.sent_ = False

    def get_nnz(self):
        return 0 if self.empty_ else self.SpMV_.get_nnz()

    def send_matrix_host_to_device(self):
        if not self.empty_:
            self.bfs_.send_matrix_host_to_device()
            if self.out_ is not None:
                self.out_.send_matrix_host_to_device()
        self.sent_ = True

    def run(self, sources=None, normalized=False, depth_hint=16):
        """-> float64[n_]: the betweenness centrality of every vertex (padding vertices: 0) summed over `sources` (an iterable of
        real vertices; None: all of them) and scaled exactly as networkx.betweenness_centrality(k=len(sources),
        endpoints=False) scales it -- 1 / ((n - 1)(n - 2)) when normalised and n > 2, otherwise 0.5 when undirected, times
        n / k when k < n -- with the factor passed to the kernel, so that no extra pass runs.  Per source: bfs_.pull_push(s, N),
        N = depth_hint, then gl_bc_accumulate on the levels still on the device.  A search whose deepest level is N + 1 may be
        truncated (the last iteration still found vertices): N is doubled, capped at n_, the source is searched again before
        anything is accumulated, and the larger N is kept for the later sources; a smaller depth proves the search finished.
        Leaves bc_, sources_, depths_ and reached_ (per source: the deepest level, the vertices of level >= 1), orphans_ (0: the
        levels are BFS results), overflowed_ (the sources whose path counts overflowed f64: they contribute nothing, a
        RuntimeWarning names them) and directed_."""
        self._require_sent()
        B, n, nr = self.backend, self.n_, self.n_real_
        src = list(range(nr)) if sources is None else [int(s) for s in sources]
        if any(s < 0 or s >= nr for s in src):
            raise ValueError("BetweennessCentrality.run(): a source outside the real vertices 0 .. %d" % (nr - 1))
        self.sources_, self.depths_, self.reached_, self.orphans_, self.overflowed_ = src, [], [], 0, []
        if self.empty_ or not src:                                   # nobody lies between two others: nothing is launched
            self.depths_, self.reached_ = [1] * len(src), [1] * len(src)
            self.bc_ = np.zeros(n, dtype=np.float64)
            return self.bc_
        scale = _bc_scale(nr, len(src), normalized, self.directed_)
        N = max(1, min(int(depth_hint), n))
        bc = B.alloc(2 * n, np.float32)                              # (n doubles)
        for i, s in enumerate(src):
            while True:
                deepest = int(self.bfs_.pull_push(s, N).max())
                if deepest < N + 1 or N >= n:
                    break
                N = min(2 * N, n)
            levels = self.bfs_.levels_[0]
            depth, reached, orphans, nonfinite = self.SpMV_.bc_accumulate(self.out_, levels, bc, scale, i > 0)
            if depth != deepest:
                raise RuntimeError("BetweennessCentrality.run(): gl_bc_accumulate saw depth %d, the search from %d returned depth %d"
                                   % (depth, s, deepest))
            self.depths_.append(depth)
            self.reached_.append(reached)
            self.orphans_ += orphans
            if nonfinite:
                self.overflowed_.append(s)
        B.sync()
        self.bc_ = B.download(bc, np.float64, n)
        if self.overflowed_:
            import warnings
            warnings.warn("BetweennessCentrality.run(): the shortest-path counts of the searches from %s overflowed f64; these sources "
                          "contribute nothing" % self.overflowed_, RuntimeWarning, stacklevel=2)
        return self.bc_


class ClosenessCentrality(_PatternApp):
    """Closeness and harmonic centrality, eccentricities and hop distances (an extension: the reference has no such driver):
    gl_msbfs, the bit-parallel breadth-first search that sweeps 64 sources at once.  The matrix is read as
    BetweennessCentrality reads it (io.simple_pattern: an edge u -> v for a stored non-zero A[v, u], u != v); the transposed
    pattern lives in a second boolean SpMVModule, out_, which exists only when the graph is directed."""
    _no_shards_ = ("gl_msbfs reads the frontier word of every column of a row, so every rank would need the whole frontier after "
                   "every level")
    BATCH = 64
    graph_ = graph_out_ = directed_ = None
    far_ = reach_ = harmonic_ = closeness_ = hops_ = sources_ = batches_ = levels_ = launches_ = None
    eccentricity_ = source_reach_ = source_far_ = diameter_ = radius_ = center_ = periphery_ = None

    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, vec_buf_len=0, comm=None, backend=None):
        _PatternApp.__init__(self, num_channels, spmv_out_buf_len, vec_buf_len, comm, backend)
        self.buf_lens_ = (spmv_out_buf_len, vec_buf_len)
        self.out_ = None                 # the transposed pattern's module (a directed graph)
        self.want_directed_ = None

    def _prepare(self, csr):
        self.graph_, self.graph_out_, self.directed_ = _bc_patterns(csr, self.want_directed_)      # (after padding)
        return self.graph_

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True, directed=None):
        """directed=None: undirected iff the pattern is symmetric; False on an asymmetric pattern takes every edge in both
        directions (io.symmetrize_simple); True keeps two plans even when the pattern is symmetric."""
        self.want_directed_ = directed
        _PatternApp.load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows)
        self.modules_ = [self.SpMV_]
        self.out_ = None
        if self.graph_out_ is not None:
            self.out_ = self.backend.SpMVModule(self.num_channels_, *self.buf_lens_)
            self.out_.set_semiring(M.LogicalSemiring)
            self.out_.set_mask_type(M.kNoMask)
            self.out_.blocking = False
            self.out_.load_and_format_matrix(self.graph_out_, skip_empty_rows)
            self.add_module(self.out_)

    def send_matrix_host_to_device(self):
        _PatternApp.send_matrix_host_to_device(self)
        if self.out_ is not None:
            self.out_.send_matrix_host_to_device()

    def run(self, sources=None, reverse=False, wf_improved=True, hops=False):
        """-> float64[n_]: the closeness centrality of every vertex (padding vertices: 0) with respect to `sources` (a sequence
        of distinct real vertices; None: all of them): reach / far, 0 where far == 0, times reach / (n_real_ - 1) with
        wf_improved, computed on the host in f64 from gl_msbfs's integer arrays -- networkx.closeness_centrality when every
        vertex is a source.  reverse=False sums at every vertex its INCOMING distances, d(s, v) over the sources s, which is
        networkx's convention on a DiGraph for closeness_centrality and harmonic_centrality; reverse=True walks the transposed
        pattern's plan and sums d(v, s).  The sources are dealt in the given order into batches of 64, one gl_msbfs call each,
        accumulating from the second on.  Leaves far_ (uint64[n_]), reach_ (uint32[n_]), harmonic_ (float64[n_]: the sum of
        1 / d, a function of the graph and the source SEQUENCE), closeness_, sources_, batches_, levels_ (the levels swept,
        summed over the batches), launches_, per source eccentricity_, source_reach_ and source_far_ (int64[len(sources)]),
        diameter_ (the largest eccentricity: exact when every vertex is a source, a lower bound otherwise), radius_ (the
        smallest), center_ and periphery_ (the sources that attain them) and, with hops=True, hops_ (uint32[len(sources), n_]:
        the distances from -- reverse: to -- every source, 0xffffffff unreached; otherwise None).  The call waits for the
        device."""
        self._require_sent()
        B, n, nr = self.backend, self.n_, self.n_real_
        src = list(range(nr)) if sources is None else [int(s) for s in sources]
        if any(s < 0 or s >= nr for s in src):
            raise ValueError("ClosenessCentrality.run(): a source outside the real vertices 0 .. %d" % (nr - 1))
        if len(set(src)) != len(src):
            raise ValueError("ClosenessCentrality.run(): a source is given twice")
        module = self.out_ if reverse and self.out_ is not None else self.SpMV_
        k_most = min(self.BATCH, max(1, len(src)))
        out = B.alloc(5 * n + (k_most * n if hops else 0), np.float32)       # (32-bit words: far, harmonic, reach, a batch's hops)
        far_buf, harmonic_buf, reach_buf = B.view(out, 0, n, 8), B.view(out, n, n, 8), B.view(out, 4 * n, n, 4)      # (first: in items)
        hops_buf = B.view(out, 5 * n, k_most * n, 4) if hops else None
        self.sources_, self.batches_, self.levels_, self.launches_ = src, 0, 0, 0
        self.hops_ = np.empty((len(src), n), dtype=np.uint32) if hops else None
        per_source = np.zeros((len(src), 3), dtype=np.int64)
        for b in range(0, len(src), self.BATCH):
            part = src[b:b + self.BATCH]
            source_stats, stats = module.msbfs(part, far_buf, reach_buf, harmonic_buf, b > 0, hops_buf)
            per_source[b:b + len(part)] = source_stats.astype(np.int64)
            self.batches_ += 1
            self.levels_ += stats[0]
            self.launches_ += stats[2]
            if hops:
                B.sync()
                self.hops_[b:b + len(part)] = B.download(hops_buf, np.uint32, len(part) * n).reshape(len(part), n)
        B.sync()
        if src:
            self.far_ = B.download(far_buf, np.uint64, n)
            self.harmonic_ = B.download(harmonic_buf, np.float64, n)
            self.reach_ = B.download(reach_buf, np.uint32, n)
        else:                                                        # no source: nothing was launched
            self.far_, self.harmonic_, self.reach_ = np.zeros(n, np.uint64), np.zeros(n, np.float64), np.zeros(n, np.uint32)
        self.source_reach_, self.source_far_, self.eccentricity_ = per_source[:, 0].copy(), per_source[:, 1].copy(), per_source[:, 2].copy()
        ecc, who = self.eccentricity_, np.asarray(src, dtype=np.int64)
        self.diameter_ = int(ecc.max()) if src else 0
        self.radius_ = int(ecc.min()) if src else 0
        self.center_ = who[ecc == self.radius_] if src else who
        self.periphery_ = who[ecc == self.diameter_] if src else who
        self.closeness_ = closeness_of(self.far_, self.reach_, nr, wf_improved)
        return self.closeness_


class Similarity(_PatternApp):
    """Neighbourhood similarity and link prediction (an extension: the reference has no such driver): gl_similarity (DESIGN.md
    4.27), the common neighbours of caller-chosen pairs of vertices -- which need not be edges -- and their sums of a weight per
    common neighbour.  The matrix is read as an undirected simple graph, as KCore reads it (io.symmetrize_simple).  The kernel
    returns integers; the weighted measures travel as fixed point (similarity_tables) and every measure is computed on the host
    in f64 from the integers (similarity_measure)."""
    _no_shards_ = "gl_similarity reads the rows of both vertices of a pair, so every rank would need the whole symmetric matrix"
    MEASURES = SIMILARITY_MEASURES
    degrees_ = graph_ = shift_ = aa_ = ra_ = aa_buf_ = ra_buf_ = None
    common_ = pairs_ = edges_ = launches_ = deferred_ = weighted_ = None

    def _prepare(self, csr):
        csr, self.degrees_ = io.symmetrize_simple(csr)
        self.graph_ = csr
        self.aa_, self.ra_, self.shift_ = similarity_tables(self.degrees_)
        return csr

    def send_matrix_host_to_device(self):
        """... and the two fixed-point weight tables, n_ 64-bit words each"""
        _PatternApp.send_matrix_host_to_device(self)
        B, n = self.backend, self.n_
        self.aa_buf_, self.ra_buf_ = B.alloc(2 * max(1, n), np.float32), B.alloc(2 * max(1, n), np.float32)
        if n:
            B.upload(self.aa_buf_, self.aa_)
            B.upload(self.ra_buf_, self.ra_)

    @classmethod
    def _measures(cls, measures):
        names = (measures,) if isinstance(measures, str) else tuple(measures)
        for name in names:
            if name not in cls.MEASURES:
                raise ValueError("Similarity: unknown measure %r (one of %s)" % (name, ", ".join(cls.MEASURES)))
        return names

    def run(self, pairs, measures=("common", "jaccard")):
        """-> {measure: array[m]} aligned with `pairs` (int[m, 2], real vertices; a pair may be an edge or not, u == v is legal).
        common is uint32, preferential_attachment uint64 (no kernel), the others float64 (similarity_measure: 0.0 where a
        denominator is 0).  gl_similarity is called once per distinct weight table needed -- at most twice, without a table
        when neither adamic_adar nor resource_allocation is asked for.  Leaves common_ (uint32[m]), pairs_ (int64[m, 2]),
        weighted_ ({measure: uint64[m]}, the fixed-point sums at shift_), deferred_ and launches_.  The call waits for the
        device."""
        names = self._measures(measures)
        self._require_sent()
        pr = np.asarray(pairs)
        if pr.size == 0:
            pr = pr.reshape(0, 2)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in "iu":
            raise ValueError("Similarity.run(): pairs must be an integer array of shape [m, 2]")
        pr = pr.astype(np.int64)
        m = pr.shape[0]
        if m and (pr.min() < 0 or pr.max() >= self.n_real_):
            raise ValueError("Similarity.run(): a pair names a vertex outside the real vertices 0 .. %d" % (self.n_real_ - 1))
        if m > 0xFFFFFFFF:
            raise ValueError("Similarity.run(): %d pairs, at most 2^32 - 1 per call" % m)
        B = self.backend
        tables = [(name, buf) for name, buf in (("adamic_adar", self.aa_buf_), ("resource_allocation", self.ra_buf_)) if name in names]
        self.pairs_, self.launches_, self.deferred_, self.weighted_ = pr, 0, 0, {}
        self.common_ = np.zeros(0, dtype=np.uint32)
        needs_kernel = any(name != "preferential_attachment" for name in names)
        if m and needs_kernel:
            out = B.alloc(5 * m, np.float32)                         # (32-bit words: the weighted sums, the pairs, the counts)
            weighted_buf, pairs_buf, common_buf = B.view(out, 0, m, 8), B.view(out, 2 * m, 2 * m, 4), B.view(out, 4 * m, m, 4)
            B.upload(pairs_buf, pr.astype(np.uint32).ravel())
            for name, table in tables or [(None, None)]:
                stats = self.SpMV_.similarity(pairs_buf, common_buf, weighted_buf if table is not None else None, table, True, m)
                self.deferred_ = stats[1]
                self.launches_ += stats[2]
                if name is not None:
                    self.weighted_[name] = B.download(weighted_buf, np.uint64, m)
            self.common_ = B.download(common_buf, np.uint32, m)
        elif needs_kernel:
            self.weighted_ = {name: np.zeros(0, dtype=np.uint64) for name, _ in tables}
        du, dv = self.degrees_[pr[:, 0]], self.degrees_[pr[:, 1]]
        return {name: similarity_measure(name, self.common_ if needs_kernel else np.zeros(m, np.uint32), du, dv,
                                         self.weighted_.get(name), self.shift_) for name in names}

    def run_edges(self, measures=("common", "jaccard")):
        """-> run() over every edge {u, v}, u < v, of the prepared graph, ascending; leaves edges_ (int64[edges, 2])"""
        self._measures(measures)
        self._require_sent()
        g = self.graph_
        rows = np.repeat(np.arange(g.num_rows, dtype=np.int64), np.diff(g.adj_indptr.astype(np.int64)))
        cols = g.adj_indices[:rows.shape[0]].astype(np.int64)
        once = cols > rows
        self.edges_ = np.stack([rows[once], cols[once]], axis=1)
        return self.run(self.edges_, measures)

    def two_hop_pairs(self, sources, limit=None):
        """-> int64[p, 2]: the distinct pairs (s, v) with v != s, v not adjacent to s and at least one common neighbour, for the
        given sources (real vertices), ordered by (s, v): the candidates of link prediction.  Host code (numpy on graph_, the prepared
        matrix -- what SpMV_.csr_matrix_ holds --, no device work), meant for a handful of sources.  Raises ValueError if more than `limit` pairs would result."""
        g = self.graph_
        if g is None:
            raise RuntimeError("Similarity.two_hop_pairs(): load_and_format_matrix first")
        ip, idx = g.adj_indptr.astype(np.int64), g.adj_indices
        src = sorted({int(s) for s in np.asarray(sources, dtype=np.int64).ravel().tolist()})
        if src and (src[0] < 0 or src[-1] >= self.n_real_):
            raise ValueError("Similarity.two_hop_pairs(): a source outside the real vertices 0 .. %d" % (self.n_real_ - 1))
        parts, total = [], 0
        for s in src:
            near = idx[ip[s]:ip[s + 1]].astype(np.int64)
            far = np.unique(np.concatenate([idx[ip[w]:ip[w + 1]] for w in near.tolist()] or [np.zeros(0, idx.dtype)])).astype(np.int64)
            far = far[(far != s) & ~np.isin(far, near)]
            total += far.shape[0]
            if limit is not None and total > limit:
                raise ValueError("Similarity.two_hop_pairs(): more than limit = %d pairs" % limit)
            parts.append(np.stack([np.full(far.shape[0], s, dtype=np.int64), far], axis=1))
        return np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int64)

    def top_k(self, source, k, measure="jaccard"):
        """-> (vertices int64[<= k], scores): the k best link candidates of `source` among two_hop_pairs([source]) by `measure`,
        ordered by (-score, vertex)"""
        (name,) = self._measures((measure,))
        self._require_sent()
        pairs = self.two_hop_pairs([source])
        scores = self.run(pairs, (name,))[name]
        order = np.lexsort((pairs[:, 1], -scores.astype(np.float64)))[:max(0, int(k))]
        return pairs[order, 1], scores[order]


class PageRank(_GraphApp):
    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, vec_buf_len=0, comm=None, backend=None):
        super().__init__(num_channels, comm, backend)
        B = self.backend
        self.semiring_ = M.ArithmeticSemiring
        self.SpMV_ = B.SpMVModule(num_channels, spmv_out_buf_len, vec_buf_len)
        self.SpMV_.set_semiring(self.semiring_)
        self.SpMV_.set_mask_type(M.kNoMask)
        self.eWiseAdd_ = B.eWiseAddModule()
        self.add_module(self.SpMV_)
        self.add_module(self.eWiseAdd_)

    def load_and_format_matrix(self, csr_float_npz_path, damping, skip_empty_rows=True):
        csr = self._load(csr_float_npz_path)
        n_real = csr.num_rows
        self._pad(csr)
        io.util_normalize_csr_matrix_by_outdegree(csr)
        csr.adj_data = (csr.adj_data * np.float32(damping)).astype(np.float32)   # app/pagerank.h:67
        self._shard(csr)
        self.SpMV_.set_row_shard(self.r0_, self.r1_)
        self.SpMV_.load_and_format_matrix(csr, skip_empty_rows)
        self.n_ = self.SpMV_.get_num_rows()
        assert self.n_ == self.SpMV_.get_num_cols()
        self.n_real_, self.damping_ = n_real, float(damping)     # (solve: the vertices that are not padding; the damping in M)
        self.dangling_bits_ = None

    def send_matrix_host_to_device(self):
        self.SpMV_.send_matrix_host_to_device()

    def pull(self, damping, num_iterations):
        B, n = self.backend, self.n_
        # rank starts at float(1.0 / n) over the PADDED n (app/pagerank.h:81), teleport is the float
        # expression (1 - damping) / n (:87)
        vector = self._new_dense(n, np.float32(1.0 / n))
        teleport = np.float32(np.float32(1) - np.float32(damping)) / np.float32(n)
        results = B.alloc(n, np.float32)
        # The reference runs SpMV with zero = 0 and then eWiseAdd(results, teleport) -> vector (app/pagerank.h:84-88).
        # The device epilogue computes zero + sum in float, so passing the teleport term AS the semiring's zero gives
        # the same float (a + b == b + a), and the two buffers swap roles instead of being copied: one launch and
        # 8n bytes less per iteration.
        if getattr(self.SpMV_, "plan_flags_", 0) & capi.GL_PLAN_REFERENCE_ORDER:
            # diagnostic run in the reference's own evaluation order: the literal module sequence, SpMV with zero = 0
            # and then eWiseAdd(teleport) (teleport + sum started from the teleport term rounds differently)
            self.SpMV_.bind_vector_buf(vector)
            self.SpMV_.bind_results_buf(results)
            self.eWiseAdd_.bind_in_buf(self._own(results))
            self.eWiseAdd_.bind_out_buf(self._own(vector))
            for _ in range(num_iterations):
                self.SpMV_.run()
                self.eWiseAdd_.run(self.r1_ - self.r0_, float(teleport))
                self._gather(vector)
            B.sync()
            return B.download_result(vector, n)
        saved = self.SpMV_.semiring_
        self.SpMV_.set_semiring(M.SemiringType(M.kMulAdd, 1.0, float(teleport)))
        # every result IS the next vector, untouched in between: the run's epilogue prepares the next run's packed x (one GPU)
        chained = (not self.comm.distributed) and hasattr(self.SpMV_, "chain") and self.SpMV_.chain(True)
        try:
            for _ in range(num_iterations):
                self.SpMV_.bind_vector_buf(vector)
                self.SpMV_.bind_results_buf(results)
                self.SpMV_.run()
                self._gather(results)
                vector, results = results, vector
        finally:
            if chained:
                self.SpMV_.chain(False)
            self.SpMV_.set_semiring(saved)
        B.sync()
        return B.download_result(vector, n)


    def _personalization(self, personalization):
        """-> p of solve(): float32[n_], >= 0, 0 on the padding vertices, normalised in f64 to sum 1 before the cast"""
        n, n0 = self.n_, self.n_real_
        p = np.zeros(n, dtype=np.float64)
        if personalization is None:
            p[:n0] = 1.0 / n0
            return p.astype(np.float32)
        given = np.asarray(personalization, dtype=np.float64)
        if given.ndim != 1 or given.shape[0] not in (n0, n):
            raise ValueError("PageRank.solve: personalization has shape %r, expected (%d,) or (%d,)" % (given.shape, n0, n))
        if not np.all(np.isfinite(given)) or np.any(given < 0):
            raise ValueError("PageRank.solve: personalization has a negative or non-finite entry")
        if np.any(given[n0:] != 0):
            raise ValueError("PageRank.solve: personalization is not 0 on the padding vertices %d..%d" % (n0, n - 1))
        total = float(np.cumsum(given[:n0])[-1])      # (in index order, like the C++ driver's loop: the same words in both)
        if not (total > 0 and np.isfinite(total)):
            raise ValueError("PageRank.solve: personalization has zero sum")
        p[:n0] = given[:n0] / total
        return p.astype(np.float32)

    def _dangling_bits(self):
        """The columns of the prepared (padded) matrix without a stored entry, one bit each: bit v % 32 of word v / 32.  From
        the column indices kept since load; built on the first solve() after a load."""
        if self.dangling_bits_ is None:
            n = self.n_
            dangling = np.bincount(self.SpMV_.csr_matrix_.adj_indices, minlength=n)[:n] == 0
            self.dangling_bits_ = np.packbits(dangling, bitorder="little").view(np.uint8)
            pad = (-self.dangling_bits_.shape[0]) % 4
            self.dangling_bits_ = np.concatenate([self.dangling_bits_, np.zeros(pad, np.uint8)]).view("<u4")
        return self.dangling_bits_

    def solve(self, damping, tol=1e-6, max_iterations=100, personalization=None, check_every=4):
        """PageRank proper (networkx's pagerank with dangling = personalization and the plain L1 change as the
        stopping rule): personalised teleport, the rank of vertices without out-edges handed back through the teleport term, and
        a residual stop.  With M the prepared matrix, D the columns of the padded matrix without an entry and p the
        personalisation (default 1 / n0 on the n0 real vertices, 0 on padding):
            x_0 = p;   c_k = float((1 - d) + d * sum_{u in D} x_k[u]);   x_{k+1} = fl32(M x_k + fl32(c_k * p));
            r_{k+1} = sum_v |x_{k+1}[v] - x_k[v]|   (sums in f64, d = float32(damping))
        until r <= tol or max_iterations.  Each iteration is the (+,x) SpMV and gl_pagerank_update; both sums stay on the
        device, `check_every` iterations are enqueued between two read-backs of the control block, and iterations enqueued
        past convergence leave the vector alone, so the result does not depend on check_every.  Leaves iterations_, converged_
        and residuals_ (float64, one per iteration run); -> float32[n_].
        ValueError: a damping other than the one the matrix was prepared with, tol < 0, check_every < 1, max_iterations
        outside [1, capi.GL_PAGERANK_MAX_SLOTS] (65536: the control block holds one residual per iteration), a personalisation
        of another length than n0 or n_, with a negative or non-finite entry, with zero sum, or non-zero on a padding vertex.
        NotImplementedError on row shards; RuntimeError before send_matrix_host_to_device."""
        if np.float32(damping) != np.float32(self.damping_):
            raise ValueError("PageRank.solve: damping %r, but the matrix was prepared with %r (load_and_format_matrix)"
                             % (damping, self.damping_))
        if not tol >= 0:
            raise ValueError("PageRank.solve: tol %r < 0" % (tol,))
        max_iterations, check_every = int(max_iterations), int(check_every)
        if max_iterations < 1 or max_iterations > capi.GL_PAGERANK_MAX_SLOTS:
            raise ValueError("PageRank.solve: max_iterations %d is not in [1, %d]" % (max_iterations, capi.GL_PAGERANK_MAX_SLOTS))
        if check_every < 1:
            raise ValueError("PageRank.solve: check_every %d < 1" % check_every)
        p = self._personalization(personalization)
        if self.comm.distributed:
            raise NotImplementedError("PageRank.solve: row shards are not supported yet (the residual and the dangling mass "
                                      "would have to be summed across ranks); use one device")
        if getattr(self.SpMV_, "plan_", None) is None:
            raise RuntimeError("PageRank.solve: the matrix is not on the device yet (send_matrix_host_to_device)")
        B, n = self.backend, self.n_
        slots = max_iterations
        p_buf = capi.DeviceBuffer.from_host(p)
        bits_buf = capi.DeviceBuffer.from_host(self._dangling_bits())
        ctl = capi.DeviceBuffer(capi.pagerank_ctl_bytes(slots))
        vector, results = B.alloc(n, np.float32), B.alloc(n, np.float32)
        capi.pagerank_begin(p_buf, n, bits_buf, vector, ctl, slots)
        saved = (self.SpMV_.semiring_, self.SpMV_.vector_buf, self.SpMV_.results_buf)
        self.SpMV_.set_semiring(self.semiring_)         # (+,x) with zero = 0; no chaining: the update rewrites every result
        done, k = False, 0
        try:
            while k < max_iterations and not done:
                for _ in range(min(check_every, max_iterations - k)):
                    k += 1
                    self.SpMV_.bind_vector_buf(vector)
                    self.SpMV_.bind_results_buf(results)
                    self.SpMV_.run()
                    capi.pagerank_update(results, vector, p_buf, bits_buf, n, damping, tol, ctl, k)
                    vector, results = results, vector
                done = bool(ctl.read(np.uint32, 1)[0])
        finally:
            self.SpMV_.set_semiring(saved[0])
            self.SpMV_.bind_vector_buf(saved[1])
            self.SpMV_.bind_results_buf(saved[2])
        done, ran, _, r = capi.pagerank_ctl_unpack(ctl.read(np.uint8, capi.pagerank_ctl_head_bytes(slots)), slots)
        self.converged_, self.iterations_ = done, ran
        self.residuals_ = r[1:ran + 1]
        return B.download_result(vector, n)

    def pull_time_breakdown(self, damping, num_iterations):
        """app/pagerank.h:93-147: pull with per-iteration wall-clock buckets (spmv, ewise, data transfer); every
        step is followed by a device sync.  Returns the rank vector (the reference returns the wrong buffer
        there); the buckets (ms per iteration) are left in `time_breakdown_` and printed."""
        B, n = self.backend, self.n_
        tb = {"spmv": 0.0, "ewise": 0.0, "data_transfer": 0.0}

        def timed(bucket, fn):
            B.sync()
            t0 = time.perf_counter()
            r = fn()
            B.sync()
            tb[bucket] += (time.perf_counter() - t0) * 1e3
            return r

        B.sync()
        t_start = time.perf_counter()
        vector = timed("data_transfer", lambda: self._new_dense(n, np.float32(1.0 / n)))
        teleport = np.float32(np.float32(1) - np.float32(damping)) / np.float32(n)
        results = B.alloc(n, np.float32)
        self.SpMV_.bind_vector_buf(vector)
        self.SpMV_.bind_results_buf(results)
        self.eWiseAdd_.bind_in_buf(self._own(results))
        self.eWiseAdd_.bind_out_buf(self._own(vector))
        own = self.r1_ - self.r0_
        for _ in range(num_iterations):
            timed("spmv", self.SpMV_.run)
            timed("ewise", lambda: self.eWiseAdd_.run(own, float(teleport)))
            timed("data_transfer", lambda: self._gather(vector))
        result = timed("data_transfer", lambda: B.download_result(vector, n))
        tb["total"] = (time.perf_counter() - t_start) * 1e3
        self.time_breakdown_ = {k: v / num_iterations for k, v in tb.items()}
        for k in ("total", "spmv", "ewise", "data_transfer"):
            print("%s_time_ms per iteration: %.4f" % (k, self.time_breakdown_[k]))
        return result


class SSSP(_GraphApp):
    def __init__(self, num_channels=M.num_hbm_channels, spmv_out_buf_len=0, spmspv_out_buf_len=0, vec_buf_len=0,
                 comm=None, backend=None, semiring=M.TropicalSemiring):
        super().__init__(num_channels, comm, backend)
        B = self.backend
        self.semiring_ = semiring
        self.SpMV_ = B.SpMVModule(num_channels, spmv_out_buf_len, vec_buf_len)
        self.SpMV_.set_semiring(self.semiring_)
        self.SpMV_.set_mask_type(M.kNoMask)
        self.SpMSpV_ = B.SpMSpVModule(spmspv_out_buf_len)
        self.SpMSpV_.set_semiring(self.semiring_)
        self.SpMSpV_.set_mask_type(M.kNoMask)
        self.SparseAssign_ = B.AssignVectorSparseModule(True)
        self.eWiseAdd_ = B.eWiseAddModule()
        for m in (self.SpMV_, self.SpMSpV_, self.SparseAssign_, self.eWiseAdd_):
            self.add_module(m)
        self.distance_ = None           # SSSP.parents(): (the last run's distances on the device, its source)
        self.orphans_ = 0

    def load_and_format_matrix(self, csr_float_npz_path, skip_empty_rows=True, weighted=False):
        """`weighted=False` is the reference's preparation (app/sssp.h:132: every weight becomes 1).  `weighted=True` (an
        extension) keeps the matrix's weights and gives every row a weight-0 diagonal entry (io.sssp_zero_diagonal)."""
        csr = self._load(csr_float_npz_path)
        if weighted:
            io.sssp_zero_diagonal(csr)
        else:
            io.sssp_add_self_edges(csr)              # app/sssp.h:132 (_preprocess)
        self._pad(csr)
        csc = io.csr2csc(csr)
        self._shard(csr)
        for m in (self.SpMV_, self.SpMSpV_):
            m.set_row_shard(self.r0_, self.r1_)
        self.SpMV_.load_and_format_matrix(csr, skip_empty_rows)
        self.SpMSpV_.load_and_format_matrix(csc)
        self.n_ = self.SpMV_.get_num_rows()
        assert self.n_ == self.SpMV_.get_num_cols()
        self.distance_ = None

    def _initial_distance(self, source):
        return self._new_dense(self.n_, self.semiring_.zero, source, 0.0)

    def _pull_loop(self, vector, first_it, num_iterations):
        B, n = self.backend, self.n_
        results = B.alloc(n, np.float32)
        # The reference copies results -> vector after every SpMV (eWiseAdd with 0, app/sssp.h:163); here the two
        # buffers swap roles instead: same values, one launch and 8n bytes less per iteration.
        chained = (not self.comm.distributed) and hasattr(self.SpMV_, "chain") and self.SpMV_.chain(True)   # (as in PageRank.pull)
        try:
            for _ in range(first_it, num_iterations + 1):
                self.SpMV_.bind_vector_buf(vector)
                self.SpMV_.bind_results_buf(results)
                self.SpMV_.run()
                self._gather(results)
                vector, results = results, vector
        finally:
            if chained:
                self.SpMV_.chain(False)
        self.distance_ = (vector, self.source_)     # SSSP.parents(): this run's distances, whole on every rank
        B.sync()
        return B.download_result(vector, n)

    def pull(self, source, num_iterations):
        self.source_ = int(source)
        return self._pull_loop(self._initial_distance(source), 1, num_iterations)

    def _start_push(self, source):
        B, n = self.backend, self.n_
        frontier = B.alloc(n + 1, capi.IDX_VAL)
        B.upload(B.view(frontier, 0, 2, 8), M.make_sparse_vec([source], [0.0]))
        distance = self._initial_distance(source)
        candidates = B.alloc(n + 1, capi.IDX_VAL)    # SpMSpV result of this shard
        self.SpMSpV_.bind_vector_buf(frontier)
        self.SpMSpV_.bind_mask_buf(distance)
        self.SpMSpV_.results_buf = candidates
        self.SparseAssign_.bind_mask_buf(candidates)
        self.SparseAssign_.bind_inout_buf(distance)
        if self.comm.distributed:
            local = B.alloc(n + 1, capi.IDX_VAL)     # relaxed entries of this shard
            self.SparseAssign_.bind_new_frontier_buf(local)
        else:
            local = None
            self.SparseAssign_.bind_new_frontier_buf(frontier)   # app/sssp.h:185-187
        return frontier, distance, candidates, local

    def _push_iteration(self, frontier, local):
        self.SpMSpV_.run()
        self.SparseAssign_.run()
        if self.comm.distributed:
            self._gather_sparse(local, frontier, self.n_, 0.0)

    def push(self, source, num_iterations):
        frontier, distance, _, local = self._start_push(source)
        for _ in range(num_iterations):
            self._push_iteration(frontier, local)
        self._gather(distance)
        self.distance_ = (distance, int(source))
        self.backend.sync()
        return self.backend.download_result(distance, self.n_)

    def send_matrix_host_to_device(self):
        self.SpMV_.send_matrix_host_to_device()
        self.SpMSpV_.send_matrix_host_to_device()
        if hasattr(self.SpMSpV_, "attach_pull"):
            self.SpMSpV_.attach_pull(self.SpMV_)     # heavy frontiers of a push iteration go row-wise

    def pull_push(self, source, num_iterations, threshold=0.05):
        """app/sssp.h:197-243, host-driven like the reference -- but the count that decides the loop is the SpMSpV's own
        completion record (gl_spmspv_wait: stored to page-locked memory by the operator's last workgroup), read while the
        relax step that was enqueued behind it runs; no copy, no stream synchronisation per iteration.  (Rounds 2-3 also had
        a device-resident schedule with both steps of every slot enqueued and one gated off: five no-op launches per slot --
        same-box it lost on five of six stand-ins, 3.60 against 3.18 ms on ogbn-products' 23 slots,
        profiles/r04_ab_schedules.txt -- retired in round 4.)"""
        n = self.n_
        self.source_ = int(source)
        frontier, distance, candidates, local = self._start_push(source)
        it = 1
        while True:
            self._push_iteration(frontier, local)
            # app/sssp.h:221 (SpMSpV result size): the run's own completion record (the relax step is already enqueued behind
            # it), or the head element's copy where there is none
            nnz = self.SpMSpV_.get_results_nnz() if not self.comm.distributed and hasattr(self.SpMSpV_, "plan_") else self.comm_sparse_count(candidates)
            if self.comm.distributed:
                import torch
                gloo = self.comm.dist.get_backend(self.comm.group) == "gloo"
                t = torch.tensor([nnz], dtype=torch.int64, device="cpu" if gloo else distance.tensor.device)
                self.comm.dist.all_reduce(t, group=self.comm.group)
                nnz = int(t.item())
            it += 1
            if not (it < num_iterations and float(nnz) / n < threshold):
                break
        self.push_iterations_ = it - 1
        self._gather(distance)
        return self._pull_loop(distance, it, num_iterations)   # app/sssp.h:227-242

    # -- predecessor tree (an extension: the reference's drivers return distances only) ---------------------------------------
    def parents(self, distance=None, source=None):
        """The shortest-path predecessor tree as uint32[n]: parent[source] = source, NO_PARENT (0xffffffff) where d[v] >= the
        semiring's zero (unreached), otherwise the SMALLEST u with a stored entry A[v, u] of weight w, d[u] < d[v] and
        (float)(d[u] + w) == d[v] -- unique, whichever mix of push / pull steps found the distances.  One pass over the CSC of
        the SpMSpV module from the finished distance vector (gl_sssp_parents): `distance=None` takes the distances and the
        source of this object's last pull / push / pull_push, which are still on the device; an array (n floats) is uploaded
        and used instead, and needs its `source`.  Row shards compute their own rows from the whole vector and all-gather the
        slices.  `orphans_` = reached vertices other than the source without such a u among this rank's rows: 0 for a
        converged result with positive weights, usually not for one cut short or for the default preparation, some of whose
        rows lack the self edge."""
        B, n = self.backend, self.n_
        if distance is None:
            if self.distance_ is None:
                raise RuntimeError("SSSP.parents(): no pull / push / pull_push has run on this object; pass the distance array and the source")
            dist, last_source = self.distance_
            source = last_source if source is None else source
        else:
            if source is None:
                raise ValueError("SSSP.parents(): a distance array needs its source")
            arr = np.ascontiguousarray(distance, dtype=np.float32)
            if arr.shape != (n,):
                raise ValueError("SSSP.parents(): the distance array has shape %s, the (padded) matrix has %d rows" % (arr.shape, n))
            dist = B.alloc(n, np.float32)
            B.upload(dist, arr)
        source = int(source)
        if not 0 <= source < n:
            raise ValueError("SSSP.parents(): source %d of %d vertices" % (source, n))
        par = B.alloc(n + 1, np.float32)      # (32-bit words: vertex numbers, then the orphan count)
        self.SpMSpV_.sssp_parents(dist, self.semiring_.zero, source, self._own(par), B.view(par, n, 1, 4))
        self._gather(par)
        B.sync()
        out = B.download(par, np.uint32, n + 1)
        self.orphans_ = int(out[n])
        return out[:n]
