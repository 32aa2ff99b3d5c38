"""CPU suite of the minimum spanning forest (gl_msf, SpMVPlan.msf, SpMVModule.msf, app.MinimumSpanningForest,
app.validate_spanning_forest, io.symmetrize_weighted): the export and its bindings exist, the host truth kept here -- Kruskal's
algorithm in the order (key(w), lo, hi) with a plain union-find, and the synchronous Boruvka round count -- agrees with networkx and
scipy, the matrix preparation does what it says, the validator accepts Kruskal's mask and refuses one violation per rule, the driver
refuses what it cannot do, and the C++ driver compiles against include/.  tests/test_gpu_msf.py compares the kernels with kruskal()
and boruvka_rounds() (kept here) bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver
from cpu_backend import CpuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSF_DRIVER = os.path.join(ROOT, "build", "msf_driver")
HEADER = "graphlily_hip_msf.h"
DECL = ("int gl_msf(gl_spmv_plan plan, const float *d_weight, uint32_t *d_in_forest, uint32_t *d_labels /* may be NULL */, "
        "uint64_t *h_stats /* may be NULL, 4 words */);")


# ------------------------------------------------------------------ the graph builders
def raw_csr(n, a, b, w):
    """the entries (a[i], b[i]) with values w[i] on n vertices as given -- one way only, duplicates kept -- sorted by (row, column)"""
    a, b, w = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(w, np.float32)
    order = np.lexsort((b, a))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, a + 1, 1)
    return io.CSRMatrix(n, n, w[order], b[order].astype(np.uint32), np.cumsum(indptr).astype(np.uint32))


def graph_of(n, a, b, w):
    """the undirected weighted graph with the edges {a[i], b[i]} of weight w[i] on n vertices, as gl_msf wants it"""
    return io.symmetrize_weighted(raw_csr(n, a, b, w))[0]


def entry_rows(sym):
    return np.repeat(np.arange(sym.num_rows, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))


def ones_of(sym):
    """the all-ones copy that is planned (the row copy stores a zero value as no entry)"""
    return io.CSRMatrix(sym.num_rows, sym.num_cols, np.ones(sym.nnz, np.float32), sym.adj_indices, sym.adj_indptr)


def mask_of(sym, lo, hi):
    """bool[nnz]: the entries (lo[i], hi[i]) and (hi[i], lo[i])"""
    n = sym.num_rows
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    want = np.concatenate([lo * n + hi, hi * n + lo])
    return np.isin(rows * n + cols, want)


def clique_edges(k, first=0):
    iu = np.triu_indices(k, 1)
    return iu[0] + first, iu[1] + first


def random_graph(n, m, seed, top=8):
    """about m edges on n vertices with integer weights 0 .. top - 1 (ties everywhere), stored one way in a random direction, some
    of them twice with different weights -> the raw CSRMatrix"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    a, b = np.concatenate([a, b[:m // 10]]), np.concatenate([b, a[:m // 10]])        # a tenth in both directions
    w = rng.integers(0, top, size=a.shape[0]).astype(np.float32)
    return raw_csr(n, a, b, w)


SPECIAL = np.array([-np.inf, -1e30, -3.5, -1e-30, -1e-45, 0.0, 1e-45, 3e-45, 1e-30, 1.0, 1e30, np.inf], dtype=np.float32)


def special_graph(n=128):
    """K_24 on 3 .. 26 with the special values dealt out over its 276 edges by a fixed permutation"""
    a, b = clique_edges(24, 3)
    w = SPECIAL[np.random.default_rng(5).permutation(a.shape[0]) % SPECIAL.shape[0]]
    return graph_of(n, a, b, w)


def components_graph(n=384):
    """a weighted K_9 on 10 .. 18, a path on 40 .. 99, a cycle on 200 .. 329; everything else, the padding included, is isolated"""
    rng = np.random.default_rng(9)
    ka, kb = clique_edges(9, 10)
    pa = np.arange(40, 99)
    ca = np.arange(200, 330)
    a, b = np.concatenate([ka, pa, ca]), np.concatenate([kb, pa + 1, np.roll(ca, -1)])
    return graph_of(n, a, b, rng.integers(0, 4, size=a.shape[0]))


# ------------------------------------------------------------------ the host truth
def keys_of(w):
    """the monotone map of f32 to uint32 that orders the weights"""
    b = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, b ^ 0xffffffff, b ^ 0x80000000)


def upper_edges(sym):
    """-> (entry numbers of the entries above the diagonal, lo, hi, 64-bit words key << 32 | entry as Python-sized ints)"""
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    up = np.flatnonzero(cols > rows)
    words = [(int(k) << 32) | int(j) for k, j in zip(keys_of(sym.adj_data[up]).tolist(), up.tolist())]
    return up, rows[up], cols[up], words


def _find(parent, x):
    while parent[x] != x:
        x = parent[x]
    return x


def kruskal(sym):
    """Kruskal's algorithm in the order (key(w), lo, hi), a plain union-find (no compression, no ranks: nothing shared with
    app._kruskal_of but the order) -> bool[nnz], both entries of every forest edge.  Reads the weights above the diagonal only."""
    up, lo, hi, words = upper_edges(sym)
    parent = list(range(sym.num_rows))
    size = [1] * sym.num_rows
    tl, th = [], []
    for _, u, v in sorted(zip(words, lo.tolist(), hi.tolist())):
        ru, rv = _find(parent, u), _find(parent, v)
        if ru != rv:
            if size[ru] < size[rv]:
                ru, rv = rv, ru
            parent[rv] = ru
            size[ru] += size[rv]
            tl.append(u)
            th.append(v)
    return mask_of(sym, tl, th)


def boruvka_rounds(sym):
    """the rounds of Boruvka's algorithm in which at least one component chooses an edge, when EVERY component chooses its
    smallest leaving edge in EVERY round: a property of graph and weights under the order"""
    up, lo, hi, words = upper_edges(sym)
    lo, hi = lo.tolist(), hi.tolist()
    comp = list(range(sym.num_rows))
    rounds = 0
    while True:
        best = {}
        for word, u, v in zip(words, lo, hi):
            cu, cv = comp[u], comp[v]
            if cu != cv:
                if best.get(cu, (word + 1,))[0] > word:
                    best[cu] = (word, u, v)
                if best.get(cv, (word + 1,))[0] > word:
                    best[cv] = (word, u, v)
        if not best:
            return rounds
        rounds += 1
        parent = {c: c for c in set(comp)}
        for _, u, v in best.values():
            ru, rv = _find(parent, comp[u]), _find(parent, comp[v])
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
        comp = [_find(parent, c) for c in comp]


def total_of(sym, mask):
    """the f64 sum of the forest's weights, once per edge, one by one in entry order"""
    once = mask & (sym.adj_indices.astype(np.int64) > entry_rows(sym))
    return float(np.cumsum(sym.adj_data[once], dtype=np.float64)[-1]) if once.any() else 0.0


def _nx_graph(sym):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(sym.num_rows))
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    up = cols > rows
    G.add_weighted_edges_from(zip(rows[up].tolist(), cols[up].tolist(), sym.adj_data[up].astype(np.float64).tolist()))
    return G


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_msf"), "libgraphlily_hip.so does not export gl_msf"
    assert len(L.gl_msf.argtypes) == 5
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_msf"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_msf" not in capi.EXPORTS and "gl_msf" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.msf) and callable(M.SpMVModule.msf)
    assert callable(app.MinimumSpanningForest.run) and callable(app.validate_spanning_forest) and callable(io.symmetrize_weighted)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "msf(DeviceBuffer weight, DeviceBuffer in_forest, uint32_t *labels = nullptr, uint64_t *stats = nullptr)" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    msf_h = open(os.path.join(ROOT, "include", "graphlily", "app", "msf.h")).read()
    for piece in ("class MinimumSpanningForest", "run(bool want_labels = false)", "total_weight()", "edges()", "weights()", "rounds()",
                  "num_components()", "util_symmetrize_weighted"):
        assert piece in msf_h
    fmt_h = open(os.path.join(ROOT, "include", "graphlily", "io", "data_formatter.h")).read()
    assert fmt_h.index("util_symmetrize_simple(") < fmt_h.index("util_symmetrize_weighted(") < fmt_h.index("util_coloring_hash(")
    assert "gl_msf.hip" in open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "msf_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_msf(None, None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


def test_keys_order_the_floats():
    """the key is monotone on the special values (given ascending), -0.0 sorts just below +0.0, and app._edge_keys is the same map"""
    k = keys_of(SPECIAL)
    assert np.all(np.diff(k) > 0) and np.all(np.diff(SPECIAL.astype(np.float64)) > 0)
    assert keys_of(np.float32(-0.0)) + 1 == keys_of(np.float32(0.0)) == 0x80000000
    rng = np.random.default_rng(3)
    w = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(keys_of(w), kind="stable"), np.argsort(w, kind="stable"))
    assert np.array_equal(app._edge_keys(w).astype(np.int64), keys_of(w))


@pytest.mark.parametrize("seed", [1, 2])
def test_kruskal_equals_networkx_on_distinct_weights(seed):
    import networkx as nx
    rng = np.random.default_rng(seed)
    n, m = 300, 1500
    a, b = rng.integers(0, n - 20, size=m), rng.integers(0, n - 20, size=m)           # (the last 20 vertices stay isolated)
    sym = graph_of(n, a, b, rng.permutation(m).astype(np.float32) - 700.0)            # distinct, some negative, one 0
    up = sym.adj_indices.astype(np.int64) > entry_rows(sym)
    assert np.unique(sym.adj_data[up]).shape[0] == np.count_nonzero(up)
    mask = kruskal(sym)
    want = {(min(u, v), max(u, v)) for u, v in nx.minimum_spanning_edges(_nx_graph(sym), algorithm="kruskal", data=False)}
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    got = set(zip(rows[mask & up].tolist(), cols[mask & up].tolist()))
    assert got == want and len(got) + nx.number_connected_components(_nx_graph(sym)) == n
    assert np.array_equal(app._kruskal_of(sym), mask)
    assert 1 <= boruvka_rounds(sym) <= 9


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_kruskal_total_equals_networkx_and_scipy_with_ties(seed):
    import networkx as nx
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    sym = io.symmetrize_weighted(random_graph(512, 3000, seed))[0]
    mask = kruskal(sym)
    total = total_of(sym, mask)
    edges = int(np.count_nonzero(mask)) // 2
    G = _nx_graph(sym)
    assert total == sum(d["weight"] for _, _, d in nx.minimum_spanning_edges(G, data=True))
    A = sp.csr_matrix((sym.adj_data.astype(np.float64) + 1.0, sym.adj_indices.astype(np.int32), sym.adj_indptr.astype(np.int32)),
                      shape=(sym.num_rows, sym.num_cols))                              # (scipy drops zero weights: shifted by + 1)
    T = minimum_spanning_tree(A)
    assert T.nnz == edges and float(T.sum()) - edges == total
    assert edges + nx.number_connected_components(G) == sym.num_rows
    assert np.array_equal(app._kruskal_of(sym), mask)


def test_closed_forms_of_the_host_truth():
    """the fixtures of tests/test_gpu_msf.py whose answer is known in closed form"""
    v = np.arange(5, 205)
    cyc = graph_of(256, v, np.roll(v, -1), np.ones(200))
    assert np.array_equal(kruskal(cyc), mask_of(cyc, v[:-2].tolist() + [5], (v[:-2] + 1).tolist() + [204]))    # all but (203, 204)
    for k in (3, 17):
        a, b = clique_edges(k, 5)
        g = graph_of(256, a, b, np.ones(a.shape[0]))
        assert np.array_equal(kruskal(g), mask_of(g, np.full(k - 1, 5), np.arange(6, 5 + k)))                  # the star at 5
    i = np.arange(1023)
    tz = np.array([(int(x) & -int(x)).bit_length() - 1 for x in i + 1], dtype=np.float32)
    path = graph_of(1024, i, i + 1, tz)
    assert kruskal(path).all() and boruvka_rounds(path) == 10
    i = np.arange(299)
    asc = graph_of(384, i, i + 1, i)
    assert kruskal(asc).all() and boruvka_rounds(asc) == 1
    assert boruvka_rounds(graph_of(128, [], [], [])) == 0


def test_symmetrize_weighted():
    nan, n = np.float32(np.nan), 8
    #            dup min     both directions   stored 0   diagonal   -0.0       a second -0.0 against +0.0
    a = np.array([0, 0, 0,    1, 2,             3,         4, 4,      5,         6, 7])
    b = np.array([1, 1, 1,    2, 1,             4,         4, 5,      6,         7, 6])
    w = np.array([5, 2, 9,    7, -3,            0,         99, 1,     -0.0,      0.0, -0.0], dtype=np.float32)
    sym, deg = io.symmetrize_weighted(raw_csr(n, a, b, w))
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    assert sym.num_rows == sym.num_cols == n and not np.any(rows == cols)
    got = {(int(r), int(c)): float(x) for r, c, x in zip(rows, cols, sym.adj_data)}
    want = {(0, 1): 2.0, (1, 2): -3.0, (3, 4): 0.0, (4, 5): 1.0, (5, 6): 0.0, (6, 7): 0.0}
    assert got == {**want, **{(c, r): x for (r, c), x in want.items()}}
    assert not np.any(np.signbit(sym.adj_data) & (sym.adj_data == 0))           # no -0.0 is left
    assert np.array_equal(deg, np.bincount(rows, minlength=n)) and deg.dtype == np.uint32
    assert np.all(np.diff(rows * n + cols) > 0)                                  # rows ascending sets
    again, _ = io.symmetrize_weighted(sym)                                       # idempotent
    assert np.array_equal(again.adj_data.view(np.uint32), sym.adj_data.view(np.uint32)) and np.array_equal(again.adj_indices, sym.adj_indices)
    with pytest.raises(ValueError, match=r"symmetrize_weighted: entry 3 \(1, 2\) is NaN"):
        io.symmetrize_weighted(raw_csr(n, a, b, np.where(np.arange(w.shape[0]) == 3, nan, w)))
    diag = np.where(np.arange(w.shape[0]) == 6, nan, w)                          # (a NaN on the diagonal goes with the diagonal)
    assert np.array_equal(io.symmetrize_weighted(raw_csr(n, a, b, diag))[0].adj_data, sym.adj_data)
    raw = random_graph(256, 900, 4)
    plain, plain_deg = io.symmetrize_weighted(raw, weighted=False)
    simple, simple_deg = io.symmetrize_simple(raw)
    assert np.array_equal(plain.adj_indices, simple.adj_indices) and np.array_equal(plain.adj_indptr, simple.adj_indptr)
    assert np.array_equal(plain.adj_data, simple.adj_data) and np.array_equal(plain_deg, simple_deg) and np.all(plain.adj_data == 1)
    assert io.symmetrize_weighted(raw)[0].nnz > plain.nnz                        # (the stored zeros are edges only when weighted)
    wide = raw_csr(8, [0], [1], [4.0])
    wide.num_cols = 16
    assert io.symmetrize_weighted(wide)[0].num_rows == 16


def test_validate_spanning_forest_accepts_kruskal_and_refuses_one_violation_per_rule():
    raw = random_graph(512, 3000, 21)
    sym = io.symmetrize_weighted(raw)[0]
    mask = kruskal(sym)
    edges = int(np.count_nonzero(mask)) // 2
    assert app.validate_spanning_forest(raw, mask) == edges == app.validate_spanning_forest(sym, mask.astype(np.uint32))
    n = sym.num_rows
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    with pytest.raises(ValueError, match="marks for the %d entries" % sym.nnz):
        app.validate_spanning_forest(raw, mask[:100])

    def both(j):
        ip = sym.adj_indptr.astype(np.int64)
        r, c = int(rows[j]), int(cols[j])
        return [j, int(ip[c] + np.searchsorted(cols[ip[c]:ip[c + 1]], r))]
    # rule 1: the two entries of an edge disagree
    j = int(np.flatnonzero(mask & (cols > rows))[7])
    bad = mask.copy()
    bad[both(j)[1]] = False
    with pytest.raises(ValueError, match=r"entry %d \(%d, %d\) is marked 1, its mirror entry 0 \(rule 1\)" % (j, rows[j], cols[j])):
        app.validate_spanning_forest(raw, bad)
    # rule 2: one edge more closes a cycle; one edge fewer no longer spans
    extra = int(np.flatnonzero(~mask & (cols > rows))[0])
    bad = mask.copy()
    bad[both(extra)] = True
    with pytest.raises(ValueError, match=r"1 of them close a cycle \(rule 2\)"):
        app.validate_spanning_forest(raw, bad)
    bad = mask.copy()
    bad[both(j)] = False
    with pytest.raises(ValueError, match=r"an edge is missing \(rule 2\)"):
        app.validate_spanning_forest(raw, bad)
    # rule 3: a forest edge swapped for an edge of EQUAL weight of the cycle it closes -- as light, spanning, acyclic, and not the one
    import networkx as nx
    up = cols > rows
    F = nx.Graph()
    F.add_edges_from(zip(rows[mask & up].tolist(), cols[mask & up].tolist()))
    entry = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(rows, cols))}
    swapped = None
    for x in np.flatnonzero(~mask & up).tolist():                            # x closes one cycle with the forest's path between its ends
        path = nx.shortest_path(F, int(rows[x]), int(cols[x]))
        same = [entry[(min(u, v), max(u, v))] for u, v in zip(path, path[1:])
                if sym.adj_data[entry[(min(u, v), max(u, v))]] == sym.adj_data[x]]
        if same:
            swapped = mask.copy()
            swapped[both(x)] = True
            swapped[both(same[0])] = False
            break
    assert swapped is not None and total_of(sym, swapped) == total_of(sym, mask) and not np.array_equal(swapped, mask)
    with pytest.raises(ValueError, match=r"and the minimum spanning forest under the order \(key\(w\), lo, hi\) (holds|leaves out) it \(rule 3\)"):
        app.validate_spanning_forest(raw, swapped)
    # weighted=False reads the matrix as symmetrize_simple does
    plain = io.symmetrize_weighted(raw, weighted=False)[0]
    assert app.validate_spanning_forest(raw, kruskal(plain), weighted=False) == n - np.unique(
        app._components_of(plain.adj_indptr, plain.adj_indices, None, n)).shape[0]


class _TwoRanks:
    """what the drivers ask of a communicator, claiming rank 0 of 2"""
    rank, world_size, distributed = 0, 2, True


def test_driver_refuses_row_shards_and_a_run_before_send(golden_dir):
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_msf reads the component"):
        app.MinimumSpanningForest(comm=_TwoRanks(), backend=CpuBackend())
    msf = app.MinimumSpanningForest(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        msf.run()
    msf.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (msf.n_, msf.n_real_) == (128, 8) and msf.graph_.nnz == 14 and msf.degrees_[:8].max() == 2
    assert np.array_equal(msf.graph_.adj_indices, io.symmetrize_weighted(msf.graph_)[0].adj_indices)
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        msf.run(labels=True)
    msf.load_and_format_matrix(raw_csr(128, [0, 1], [1, 2], [0.0, 3.0]), True, weighted=False)
    assert msf.graph_.nnz == 2 and np.all(msf.graph_.adj_data == 1)
    msf.load_and_format_matrix(raw_csr(128, [0, 1], [1, 2], [0.0, 3.0]))
    assert msf.graph_.nnz == 4 and sorted(msf.graph_.adj_data.tolist()) == [0.0, 0.0, 3.0, 3.0]


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("msf_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([MSF_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
