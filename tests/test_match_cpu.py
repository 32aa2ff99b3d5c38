"""CPU suite of the greedy weighted matching (gl_match, SpMVPlan.match, SpMVModule.match, app.Matching, app.validate_matching,
io.symmetrize_weighted's keep="largest"): the export and its bindings exist, the two host truths kept here -- greedy() over the
edges sorted by (~key(w), lo, hi), and pointer_rounds(), the locally dominant matching run round by round as the kernels run it
-- agree with each other and with app._greedy_matching_of on every graph tests/test_gpu_match.py uses, the result is maximal
and at least half the optimum (networkx), the matrix preparation does what it says, the validator accepts the truth and refuses
one violation per rule, the driver refuses what it cannot do, and the C++ driver compiles against include/.
tests/test_gpu_match.py compares the kernels with greedy() and pointer_rounds() (kept here) bit for bit."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver
from cpu_backend import CpuBackend
from test_msf_cpu import SPECIAL, clique_edges, components_graph, entry_rows, graph_of, keys_of, random_graph, raw_csr, special_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH_DRIVER = os.path.join(ROOT, "build", "match_driver")
HEADER = "graphlily_hip_match.h"
DECL = "int gl_match(gl_spmv_plan plan, const float *d_weight, uint32_t *d_mate, uint64_t *h_stats /* may be NULL, 4 words */);"
FREE = 0xffffffff


# ------------------------------------------------------------------ the host truth
def greedy(sym):
    """the greedy matching: the edges sorted by (~key(w), lo, hi) as plain tuples, an edge kept iff both its ends are free ->
    uint32[n] mates, FREE for a free vertex"""
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    up = cols > rows
    inv = 0xffffffff - keys_of(sym.adj_data[up])
    mate = [FREE] * sym.num_rows
    for _, lo, hi in sorted(zip(inv.tolist(), rows[up].tolist(), cols[up].tolist())):
        if mate[lo] == FREE and mate[hi] == FREE:
            mate[lo], mate[hi] = hi, lo
    return np.asarray(mate, dtype=np.uint32)


def pointer_rounds(sym):
    """the locally dominant matching, round by round (written without a look at app._greedy_matching_of): every listed vertex
    points to its best free neighbour under (~key(w), lo, hi); two vertices that point to each other are matched; the free
    vertices that pointed to a freshly matched vertex are the next round's list; round 1 lists every vertex with a row
    -> (uint32[n] mates, rounds with a non-empty list, row scans)"""
    n = sym.num_rows
    indptr = sym.adj_indptr.astype(np.int64).tolist()
    cols = sym.adj_indices.astype(np.int64).tolist()
    inv = (0xffffffff - keys_of(sym.adj_data)).tolist() if sym.nnz else []
    mate, cand = [FREE] * n, [FREE] * n
    todo = [v for v in range(n) if indptr[v + 1] > indptr[v]]
    rounds = scans = 0
    while todo:
        rounds += 1
        scans += len(todo)
        for v in todo:
            best = None
            for j in range(indptr[v], indptr[v + 1]):
                u = cols[j]
                if u != v and u < n and mate[u] == FREE:
                    t = (inv[j], min(u, v), max(u, v), u)
                    if best is None or t < best:
                        best = t
            cand[v] = FREE if best is None else best[3]
        fresh = []
        for v in todo:
            u = cand[v]
            if u != FREE and cand[u] == v:
                for x, y in ((v, u), (u, v)):
                    if mate[x] == FREE:
                        mate[x] = y
                        fresh.append(x)
        todo = [w for x in fresh for w in cols[indptr[x]:indptr[x + 1]] if w < n and mate[w] == FREE and cand[w] == x]
        assert len(set(todo)) == len(todo), "a vertex has one pointer: it is found once"
    return np.asarray(mate, dtype=np.uint32), rounds, scans


def weight_of(sym, mate):
    """the f64 sum of the matched edges' weights, once per edge, one by one in entry order"""
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    once = (np.asarray(mate).astype(np.int64)[rows] == cols) & (cols > rows)
    return float(np.cumsum(sym.adj_data[once], dtype=np.float64)[-1]) if once.any() else 0.0


def _nx_graph(sym):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(sym.num_rows))
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    up = cols > rows
    G.add_weighted_edges_from(zip(rows[up].tolist(), cols[up].tolist(), sym.adj_data[up].astype(np.float64).tolist()))
    return G


def pairs_of(mate):
    m = np.asarray(mate).astype(np.int64)
    return {(int(v), int(m[v])) for v in np.flatnonzero((m != FREE) & (np.arange(m.shape[0]) < m))}


# ------------------------------------------------------------------ the graphs of tests/test_gpu_match.py
def mate_of_pairs(n, lo, hi):
    mate = np.full(n, FREE, dtype=np.uint32)
    mate[np.asarray(lo)], mate[np.asarray(hi)] = np.asarray(hi), np.asarray(lo)
    return mate


def path_graph(ascending):
    """the path 0 - 1 - ... - 599 on 640 vertices, w(i, i + 1) = i or every weight 1"""
    i = np.arange(599)
    return graph_of(640, i, i + 1, i if ascending else np.ones(599))


def clique_graph(k):
    a, b = clique_edges(k, 5)
    return graph_of(256, a, b, np.ones(a.shape[0]))


def star_graph(distinct):
    """hub 11, leaves 12 .. 5011"""
    return graph_of(5120, np.full(5000, 11), np.arange(12, 5012), np.arange(5000)[::-1] if distinct else np.ones(5000))


def hubs_graph(w01):
    """two hubs 0 and 1 over the leaves 2 .. 5001 (every such edge of weight 1), and the edge (0, 1) of weight w01"""
    leaves = np.arange(2, 5002)
    a, b = np.concatenate([[0], np.zeros(5000, np.int64), np.ones(5000, np.int64)]), np.concatenate([[1], leaves, leaves])
    return graph_of(5120, a, b, np.concatenate([[w01], np.ones(10000)]))


def largest_of(raw):
    return io.symmetrize_weighted(raw, keep="largest")[0]


def distinct_copy(sym, seed=3):
    """the same pattern with all-distinct weights, both entries of an edge alike"""
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    edge = np.minimum(rows, cols) * sym.num_rows + np.maximum(rows, cols)
    uniq, inverse = np.unique(edge, return_inverse=True)
    w = np.random.default_rng(seed).permutation(uniq.shape[0]).astype(np.float32)[inverse] - 1000.0
    return io.CSRMatrix(sym.num_rows, sym.num_cols, w, sym.adj_indices, sym.adj_indptr)


@functools.lru_cache(maxsize=None)
def gpu_graph(name):
    """-> (symmetric weighted matrix, greedy() mates, pointer_rounds() rounds, scans): computed once, shared, never written"""
    if name in ("path_ascending", "path_equal"):
        sym = path_graph(name == "path_ascending")
    elif name.startswith("clique_"):
        sym = clique_graph(int(name[7:]))
    elif name in ("star_distinct", "star_equal"):
        sym = star_graph(name == "star_distinct")
    elif name in ("hubs_heaviest", "hubs_lightest"):
        sym = hubs_graph(2.0 if name == "hubs_heaviest" else 0.5)
    elif name == "special":
        sym = special_graph()
    elif name == "components":
        sym = components_graph()
    elif name.startswith("random_"):
        sym = largest_of(random_graph(4096, 20000, int(name[7:])))
    elif name == "mid":
        sym = largest_of(random_graph(1536, 9000, 40, top=5))
    elif name == "wide":
        sym = largest_of(random_graph(40960, 100000, 7))
    elif name == "mid_distinct":
        sym = distinct_copy(gpu_graph("mid")[0])
    else:
        raise KeyError(name)
    mate, rounds, scans = pointer_rounds(sym)
    want = greedy(sym)
    assert np.array_equal(mate, want), "%s: the pointer rounds and the greedy pass disagree" % name
    want.setflags(write=False)
    return sym, want, rounds, scans


GPU_GRAPHS = ["path_ascending", "path_equal", "clique_3", "clique_17", "clique_65", "clique_130", "star_distinct", "star_equal",
              "hubs_heaviest", "hubs_lightest", "special", "components", "random_1", "random_2", "mid", "mid_distinct", "wide"]


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_match"), "libgraphlily_hip.so does not export gl_match"
    assert len(L.gl_match.argtypes) == 4
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_match"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_match" not in capi.EXPORTS and "gl_match" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.match) and callable(M.SpMVModule.match)
    assert callable(app.Matching.run) and callable(app.validate_matching) and callable(app._greedy_matching_of)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "match(DeviceBuffer weight, DeviceBuffer mate, uint64_t *stats = nullptr)" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    match_h = open(os.path.join(ROOT, "include", "graphlily", "app", "matching.h")).read()
    for piece in ("class Matching", "run()", "mate()", "edges()", "weights()", "total_weight()", "num_matched()", "rounds()", "scans()",
                  "util_symmetrize_weighted"):
        assert piece in match_h
    fmt_h = open(os.path.join(ROOT, "include", "graphlily", "io", "data_formatter.h")).read()
    assert "bool keep_largest = false" in fmt_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_match.hip" in make and HEADER in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "match_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_match(None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


@pytest.mark.parametrize("name", GPU_GRAPHS)
def test_host_truths_agree_on_every_gpu_graph(name):
    """greedy(), pointer_rounds() and app._greedy_matching_of give one matching; it is an involution over edges and maximal"""
    import networkx as nx
    sym, want, rounds, scans = gpu_graph(name)
    assert np.array_equal(app._greedy_matching_of(sym), want)
    assert app.validate_matching(sym, want) == len(pairs_of(want))
    assert nx.is_maximal_matching(_nx_graph(sym), pairs_of(want))
    listed = int(np.count_nonzero(np.diff(sym.adj_indptr.astype(np.int64))))
    assert rounds >= 1 and scans >= listed and rounds <= len(pairs_of(want)) + 1


def test_closed_forms_of_the_host_truth():
    """the fixtures of tests/test_gpu_match.py whose answer is known in closed form"""
    lo = np.arange(0, 600, 2)
    sym, want, rounds, scans = gpu_graph("path_ascending")                 # heaviest first: (598, 599), (596, 597), ...
    assert np.array_equal(want, mate_of_pairs(640, lo, lo + 1)) and (rounds, scans) == (300, 899)
    sym, want, rounds, scans = gpu_graph("path_equal")                     # smallest (lo, hi) first: (0, 1), (2, 3), ...
    assert np.array_equal(want, mate_of_pairs(640, lo, lo + 1)) and (rounds, scans) == (300, 899)
    odd = graph_of(128, np.arange(6), np.arange(6) + 1, np.arange(6))      # 7 vertices, ascending: 0 stays free
    assert pairs_of(greedy(odd)) == {(1, 2), (3, 4), (5, 6)}
    for k in (3, 17, 65, 130):                                             # K_k, equal weights: (5, 6), (7, 8), ... one pair a round
        sym, want, rounds, scans = gpu_graph("clique_%d" % k)
        lo = 5 + np.arange(0, k - 1, 2)
        assert np.array_equal(want, mate_of_pairs(256, lo, lo + 1))
        assert rounds == (k + 1) // 2 and scans == sum(k - 2 * i for i in range((k + 1) // 2))
    assert gpu_graph("clique_130")[2:] == (65, 4290)
    for name, leaf in (("star_distinct", 12), ("star_equal", 12)):        # the heaviest leaf is the first, and so is the smallest
        sym, want, rounds, scans = gpu_graph(name)
        assert np.array_equal(want, mate_of_pairs(5120, [11], [leaf])) and (rounds, scans) == (2, 10000)
    assert pairs_of(gpu_graph("hubs_heaviest")[1]) == {(0, 1)}
    assert pairs_of(gpu_graph("hubs_lightest")[1]) == {(0, 2), (1, 3)}
    none = graph_of(128, [], [], [])
    assert pointer_rounds(none)[1:] == (0, 0) and not pairs_of(greedy(none))


def test_order_is_heaviest_first_by_key():
    """on the special values (given ascending) the heavier edge wins: a path a - b - c takes its heavier edge"""
    for i in range(SPECIAL.shape[0] - 1):
        g = graph_of(128, [0, 1], [1, 2], [SPECIAL[i], SPECIAL[i + 1]])
        assert pairs_of(greedy(g)) == {(1, 2)} == pairs_of(pointer_rounds(g)[0])
    g = graph_of(128, [0, 1], [1, 2], [2.0, 2.0])                          # a tie: the smallest (lo, hi)
    assert pairs_of(greedy(g)) == {(0, 1)}


def test_half_approximation_and_maximality_against_networkx():
    """200 random graphs of 4 .. 40 vertices with integer weights 1 .. 6: twice the greedy weight is at least the optimum's, and
    the result is a maximal matching"""
    import networkx as nx
    rng = np.random.default_rng(2024)
    worst = 1.0
    for _ in range(200):
        n = int(rng.integers(4, 41))
        m = int(rng.integers(n, 3 * n))
        a, b = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
        sym = largest_of(raw_csr(64, a, b, rng.integers(1, 7, size=m)))
        mate, _, _ = pointer_rounds(sym)
        assert np.array_equal(mate, greedy(sym)) and np.array_equal(mate, app._greedy_matching_of(sym))
        G = _nx_graph(sym)
        assert nx.is_maximal_matching(G, pairs_of(mate))
        best = sum(G[u][v]["weight"] for u, v in nx.max_weight_matching(G))
        got = weight_of(sym, mate)
        assert 2.0 * got >= best
        if best > 0:
            worst = min(worst, got / best)
    assert worst >= 0.5


def test_symmetrize_weighted_keeps_the_largest_on_request():
    n = 8
    #            stored three times   both directions   -0.0 against +0.0    once
    a = np.array([0, 0, 0,             1, 2,             6, 7,                3])
    b = np.array([1, 1, 1,             2, 1,             7, 6,                4])
    w = np.array([5, 2, 9,             7, -3,            0.0, -0.0,           -4], dtype=np.float32)
    raw = raw_csr(n, a, b, w)

    def as_dict(sym):
        return {(int(r), int(c)): float(x) for r, c, x in zip(entry_rows(sym), sym.adj_indices, sym.adj_data)}
    large, deg = io.symmetrize_weighted(raw, keep="largest")
    want = {(0, 1): 9.0, (1, 2): 7.0, (6, 7): 0.0, (3, 4): -4.0}
    assert as_dict(large) == {**want, **{(c, r): x for (r, c), x in want.items()}}
    assert not np.any(np.signbit(large.adj_data) & (large.adj_data == 0)) and deg.dtype == np.uint32
    small = io.symmetrize_weighted(raw, keep="smallest")[0]
    want = {(0, 1): 2.0, (1, 2): -3.0, (6, 7): 0.0, (3, 4): -4.0}
    assert as_dict(small) == {**want, **{(c, r): x for (r, c), x in want.items()}}
    default = io.symmetrize_weighted(raw)[0]                                # the default is unchanged
    assert np.array_equal(default.adj_data.view(np.uint32), small.adj_data.view(np.uint32))
    assert np.array_equal(default.adj_indices, large.adj_indices) and np.array_equal(default.adj_indptr, large.adj_indptr)
    inf = io.symmetrize_weighted(raw_csr(n, [0, 1], [1, 0], [-np.inf, np.inf]), keep="largest")[0]
    assert inf.adj_data.tolist() == [np.inf, np.inf]
    with pytest.raises(ValueError, match="keep is 'middle'"):
        io.symmetrize_weighted(raw, keep="middle")
    with pytest.raises(ValueError, match=r"symmetrize_weighted: entry 1 \(0, 1\) is NaN"):
        io.symmetrize_weighted(raw_csr(n, a, b, np.where(np.arange(8) == 1, np.float32(np.nan), w)), keep="largest")
    plain = io.symmetrize_weighted(raw, weighted=False, keep="largest")    # weighted=False: symmetrize_simple's reading
    assert np.all(plain[0].adj_data == 1) and np.array_equal(plain[0].adj_indices, io.symmetrize_simple(raw)[0].adj_indices)


def _loaded(m, **kw):
    d = app.Matching(backend=CpuBackend())
    d.load_and_format_matrix(m, True, **kw)
    return d


def test_driver_prepares_the_graph_and_refuses_what_it_cannot_do(golden_dir):
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_match reads the mate"):
        app.Matching(comm=TwoRanks(), backend=CpuBackend())
    d = app.Matching(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (d.n_, d.n_real_) == (128, 8) and d.graph_.nnz == 14 and d.degrees_[:8].max() == 2
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    raw = raw_csr(128, [0, 0, 1, 2, 3, 4], [1, 1, 2, 3, 4, 5], [1.0, 4.0, 0.0, -2.0, 3.0, -0.0])
    d = _loaded(raw)                                                       # keep="largest"; a stored 0 and a negative weight are edges
    assert d.graph_.nnz == 10 and sorted(d.graph_.adj_data[d.graph_.adj_indices > entry_rows(d.graph_)].tolist()) == [-2.0, 0.0, 0.0, 3.0, 4.0]
    assert not np.any(np.signbit(d.graph_.adj_data) & (d.graph_.adj_data == 0))
    d = _loaded(raw, drop_nonpositive=True)                                # only (0, 1) and (3, 4) stay
    assert d.graph_.nnz == 4 and sorted(d.graph_.adj_data.tolist()) == [3.0, 3.0, 4.0, 4.0]
    assert d.graph_.adj_indices.tolist() == [1, 0, 4, 3] and d.degrees_[:6].tolist() == [1, 1, 0, 1, 1, 0]
    assert d.graph_.adj_indptr[-1] == 4 and d.graph_.num_rows == 128
    d = _loaded(raw, weighted=False)                                       # KCore's reading: zero values are no edges, weights 1
    assert d.graph_.nnz == 6 and np.all(d.graph_.adj_data == 1)
    assert np.array_equal(d.graph_.adj_indices, io.symmetrize_simple(raw)[0].adj_indices)
    with pytest.raises(ValueError, match="is NaN"):
        _loaded(raw_csr(128, [0, 1], [1, 2], [1.0, np.nan]))
    # signed data: with the non-positive edges the greedy matching takes (1, 2) of weight -1 last; without them it does not
    signed = raw_csr(128, [0, 1, 3], [1, 2, 4], [-5.0, -1.0, 2.0])
    assert pairs_of(greedy(_loaded(signed).graph_)) == {(1, 2), (3, 4)}
    assert pairs_of(greedy(_loaded(signed, drop_nonpositive=True).graph_)) == {(3, 4)}


def test_validate_matching_accepts_the_truth_and_refuses_one_violation_per_rule():
    raw = random_graph(512, 3000, 21)
    sym = largest_of(raw)
    want = greedy(sym)
    pairs = len(pairs_of(want))
    assert app.validate_matching(raw, want) == pairs == app.validate_matching(sym, want.astype(np.int64))
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    with pytest.raises(ValueError, match="mates for the 512 vertices"):
        app.validate_matching(raw, want[:100])
    v = int(np.flatnonzero((want != FREE) & (np.arange(512) < want))[5])   # a pair v < u
    u = int(want[v])
    # rule 1: not an involution -- one end forgets its partner; a vertex matched to itself; a mate that is no vertex
    bad = want.copy()
    bad[u] = FREE
    with pytest.raises(ValueError, match=r"vertex %d is matched to %d, which is free \(rule 1\)" % (v, u)):
        app.validate_matching(raw, bad)
    bad = want.copy()
    bad[v] = v
    with pytest.raises(ValueError, match=r"vertex %d is matched to %d, which is itself \(rule 1\)" % (v, v)):
        app.validate_matching(raw, bad)
    bad = want.copy()
    bad[v] = 512
    with pytest.raises(ValueError, match=r"which is no vertex \(rule 1\)"):
        app.validate_matching(raw, bad)
    # rule 2: two free vertices that share no edge are paired
    free = np.flatnonzero(want == FREE)
    assert free.shape[0] >= 2
    x, y = int(free[0]), int(free[1])
    assert not np.any((rows == x) & (cols == y))                           # (free vertices of a maximal matching are not adjacent)
    bad = want.copy()
    bad[x], bad[y] = y, x
    with pytest.raises(ValueError, match=r"vertex %d is matched to %d, and \(%d, %d\) is no edge of the graph \(rule 2\)" % (x, y, x, y)):
        app.validate_matching(raw, bad)
    # rule 3: a pair taken apart leaves an edge with two free ends
    bad = want.copy()
    bad[u] = bad[v] = FREE
    with pytest.raises(ValueError, match=r"both ends of edge \(%d, %d\) .* are free: the matching is not maximal \(rule 3\)" % (v, u)):
        app.validate_matching(raw, bad)
    # rule 4: another maximal matching -- the greedy one of the same graph with other weights
    other = greedy(io.CSRMatrix(sym.num_rows, sym.num_cols, -sym.adj_data, sym.adj_indices, sym.adj_indptr))
    assert not np.array_equal(other, want)
    with pytest.raises(ValueError, match=r"in the greedy matching under the order \(~key\(w\), lo, hi\) it is (free|matched to \d+) \(rule 4\)"):
        app.validate_matching(raw, other)
    # weighted=False and drop_nonpositive read the matrix as the driver does
    plain = io.symmetrize_weighted(raw, weighted=False)[0]
    assert app.validate_matching(raw, greedy(plain), weighted=False) == len(pairs_of(greedy(plain)))
    signed = io.CSRMatrix(raw.num_rows, raw.num_cols, raw.adj_data - 3.0, raw.adj_indices, raw.adj_indptr)
    pos = app._matching_graph_of(signed, True, True)[0]
    assert 0 < pos.nnz < largest_of(signed).nnz and np.all(pos.adj_data > 0)
    assert app.validate_matching(signed, greedy(pos), drop_nonpositive=True) == len(pairs_of(greedy(pos)))
    with pytest.raises(ValueError, match=r"\(rule [34]\)"):
        app.validate_matching(signed, greedy(pos))


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("match_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([MATCH_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference


def test_walk_stars_one_entry_of_every_hub_row_decides():
    """the inputs of tests/test_gpu_walk.py::test_match: with the hub's last entry (ascending weights) or its first (descending)
    and the mirror removed, every hub with two leaves or more is matched to somebody else -- a walk that skips that entry cannot
    give the expected mates; and the closed forms of the whole graph"""
    from test_gpu_walk import DEGREES, N, _stars, match_stars, star_hubs
    hubs, last = star_hubs(1), _stars()[4]
    two = np.asarray(DEGREES)[np.asarray(DEGREES) > 0] >= 2
    for ascending, drop in ((True, "last"), (False, "first")):
        sym, want, rounds, scans = match_stars(ascending)
        partner = last if ascending else hubs + 1
        assert np.array_equal(want, mate_of_pairs(N, hubs, partner)) and (rounds, scans) == (2, 2536 + 2519 - 17)
        less = match_stars(ascending, drop)
        assert less[0].nnz == sym.nnz - 2 * 17 and np.all(less[1][hubs[two]] != partner[two]) and np.all(less[1][hubs[two]] != FREE)
        assert np.all(less[1][partner] == FREE) and less[3] < scans
