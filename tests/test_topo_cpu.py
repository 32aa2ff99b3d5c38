"""CPU suite of the topological levels and critical paths (gl_topo, SpMVPlan.topo, SpMVModule.topo, app.TopologicalOrder,
app.validate_topological, io.directed_weighted): the export and its bindings exist, the host model -- a plain level-synchronous
loop that visits the predecessors in ascending order -- meets networkx and the closed forms on every named case,
io.directed_weighted keeps every rule of its reading, the validator accepts the truth and refuses one violation per rule, the
driver prepares both patterns and refuses what it cannot do, the golden fixture is the model's, and the C++ driver compiles against
include/.  tests/test_gpu_topo.py compares the kernels with topo_model (kept here) on the cases of topo_case.

Everything the model returns is a function of (graph, weights): level, dist and parent are compared as 32-bit words."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver
from test_cc_cpu import permute_rows
from test_kcore_cpu import _csr
from test_scc_cpu import scc_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPO_DRIVER = os.path.join(ROOT, "build", "topo_driver")
HEADER = "graphlily_hip_topo.h"
DECL = ("int gl_topo(gl_spmv_plan plan_in, gl_spmv_plan plan_out /* == plan_in: symmetric */, const float *d_weight /* may be NULL: unweighted */, "
        "uint32_t *d_level, uint32_t *d_order /* may be NULL */, float *d_dist /* given iff d_weight is */, "
        "uint32_t *d_parent /* given iff d_weight is */, uint64_t *h_stats /* may be NULL, 4 words: peeled, levels, widest, launches */);")
GOLDEN, EXPECTED = "topo_layered_csr_float32.npz", "topo_layered_expected.npz"
NONE = 0xFFFFFFFF
NAN_BITS = 0x7FC00000


# ------------------------------------------------------------------ the host model
def topo_model(n, src, dst, w=None):
    """The definition, one level at a time in plain loops, on the edges src[i] -> dst[i] (simple: no loops, no duplicates) with
    the f32 weights w[i] -> (level uint32[n], dist float32[n] or None, parent uint32[n] or None, (peeled, levels, widest)).  The
    predecessors of a vertex are visited in ascending order and a candidate replaces the best one only when it is > it: the
    smallest predecessor that attains the maximum stays."""
    src, dst = [int(x) for x in src], [int(x) for x in dst]
    preds, succs = [[] for _ in range(n)], [[] for _ in range(n)]
    for i in sorted(range(len(src)), key=lambda i: (dst[i], src[i])):
        preds[dst[i]].append((src[i], None if w is None else np.float32(w[i])))
        succs[src[i]].append(dst[i])
    pending = [len(p) for p in preds]
    level = np.full(n, NONE, np.uint32)
    dist = parent = None
    if w is not None:
        dist = np.full(n, NAN_BITS, np.uint32).view(np.float32)
        parent = np.full(n, NONE, np.uint32)
    front = [v for v in range(n) if pending[v] == 0]
    peeled = levels = widest = 0
    with np.errstate(over="ignore"):
        while front:
            peeled, levels, widest = peeled + len(front), levels + 1, max(widest, len(front))
            nxt = []
            for v in front:
                level[v] = levels - 1
                if w is not None:
                    best, who = np.float32(0.0), NONE
                    for k, (u, wt) in enumerate(preds[v]):
                        cand = np.float32(dist[u] + wt)
                        if k == 0 or cand > best:
                            best, who = cand, u
                    dist[v], parent[v] = best, who
            for v in front:                                       # (every dist of the level is final before the next one reads it)
                for x in succs[v]:
                    pending[x] -= 1
                    if pending[x] == 0:
                        nxt.append(x)
            front = nxt
    return level, dist, parent, (peeled, levels, widest)


# ------------------------------------------------------------------ the named cases
FAN_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513)


def _edges(name):
    """-> (n, src, dst) of the named graph, plainly numbered"""
    if name == "path_600":
        s = np.arange(599)
        return 640, s, s + 1
    if name == "path_desc_600":
        s = np.arange(599)
        return 640, s + 1, s
    if name == "tournament_70":
        i, j = np.divmod(np.arange(70 * 70), 70)
        return 96, i[i < j], j[i < j]
    if name == "in_hub_1000":
        return 1024, np.arange(1, 1001), np.zeros(1000, np.int64)
    if name == "out_hub_1000":
        return 1024, np.zeros(1000, np.int64), np.arange(1, 1001)
    if name == "fan_lengths":                                       # 520 sources; row 520 + i has FAN_LENGTHS[i] of them
        s = np.concatenate([(37 * i + np.arange(k)) % 520 for i, k in enumerate(FAN_LENGTHS)])
        d = np.concatenate([np.full(k, 520 + i) for i, k in enumerate(FAN_LENGTHS)])
        return 540, s, d
    if name == "grid_24x24":
        i, j = np.divmod(np.arange(576), 24)
        v = np.arange(576)
        return 576, np.concatenate([v[j < 23], v[i < 23]]), np.concatenate([v[j < 23] + 1, v[i < 23] + 24])
    if name == "tree_1023":
        c = np.arange(1, 1023)
        return 1023, (c - 1) // 2, c
    if name == "layered_2000_6000":
        rng = np.random.default_rng(5)
        layer = rng.integers(0, 40, 2000)
        e = rng.integers(0, 2000, (9000, 2))
        e = e[layer[e[:, 0]] < layer[e[:, 1]]]
        e = np.unique(e, axis=0)[:6000]
        return 2000, e[:, 0], e[:, 1]
    if name == "cycle_5":
        s = np.arange(5)
        return 5, s, (s + 1) % 5
    if name == "lollipop":                                          # 0 -> .. -> 9 -> the cycle 10 .. 19 -> 20 -> .. -> 29
        s = np.arange(29)
        return 30, np.concatenate([s, [19]]), np.concatenate([s + 1, [10]])
    if name == "symmetric":                                         # a triangle, seven isolated vertices
        return 10, np.array([0, 1, 1, 2, 2, 0]), np.array([1, 0, 2, 1, 0, 2])
    if name == "empty":
        return 64, np.zeros(0, np.int64), np.zeros(0, np.int64)
    raise KeyError(name)


ACYCLIC = ["path_600", "path_desc_600", "tournament_70", "tournament_70_perm", "in_hub_1000", "in_hub_1000_perm", "out_hub_1000",
           "out_hub_1000_perm", "fan_lengths", "fan_lengths_perm", "grid_24x24", "grid_24x24_perm", "tree_1023", "tree_1023_perm",
           "layered_2000_6000_perm"]
CYCLIC = ["cycle_5", "lollipop", "lollipop_perm", "symmetric", "bowtie", "random_1000_1400"]
CASES = ACYCLIC + CYCLIC + ["empty"]
WEIGHTS = ("equal", "signed", "fractions", "subnormal", "huge", "huge_pos", "huge_neg", "peak_first", "peak_last", "ties")


@functools.lru_cache(maxsize=None)
def topo_case(name):
    """-> (csr_in, csr_out or None, src, dst): the patterns as io.simple_pattern prepares them (every value 1; csr_out None only
    for `symmetric`) and the edges in the order of csr_in's entries; read-only arrays, shared by both test files"""
    if name in ("bowtie", "random_1000_1400"):
        cin, cout = scc_case(name)[:2]
    else:
        n, s, d = _edges(name[:-5] if name.endswith("_perm") else name)
        if name.endswith("_perm"):
            where = np.random.default_rng(len(name)).permutation(n)
            s, d = where[s], where[d]
        cin, cout, _ = io.simple_pattern(_csr(n, d, s))             # an entry A[v, u] is the edge u -> v
        assert (cout is None) == (name in ("symmetric", "empty"))
        if name == "empty":
            cout = cin.copy()
    dst = np.repeat(np.arange(cin.num_rows, dtype=np.int64), np.diff(cin.adj_indptr.astype(np.int64)))
    src = cin.adj_indices.astype(np.int64)
    for m in (cin, cout):
        if m is not None:
            for arr in (m.adj_indptr, m.adj_indices, m.adj_data):
                arr.setflags(write=False)
    for arr in (src, dst):
        arr.setflags(write=False)
    return cin, cout, src, dst


@functools.lru_cache(maxsize=None)
def topo_weights(name, kind):
    """-> float32[nnz] aligned with csr_in's entries (row v, ascending u): finite, no -0.0"""
    cin, _, src, dst = topo_case(name)
    m = src.shape[0]
    rng = np.random.default_rng(WEIGHTS.index(kind) + 100)
    ip = cin.adj_indptr.astype(np.int64)
    first, length = ip[dst], (ip[dst + 1] - ip[dst])
    at = np.arange(m) - first                                      # the entry's place in its row
    if kind == "equal":
        w = np.ones(m)
    elif kind == "signed":
        w = rng.integers(-3, 4, m).astype(np.float64)
    elif kind == "fractions":
        w = rng.integers(1, 10, m) * np.float32(0.1)
    elif kind == "subnormal":
        w = rng.integers(1, 1000, m) * 1e-42
    elif kind == "huge":                                           # 12 steps one way overflow
        w = np.where(rng.integers(0, 2, m) > 0, 3e37, -3e37)
    elif kind == "huge_pos":
        w = np.full(m, 3e37)
    elif kind == "huge_neg":
        w = np.full(m, -3e37)
    elif kind == "peak_first":                                     # the maximum at the first entry of every row
        w = np.where(at == 0, 5.0, 1.0)
    elif kind == "peak_last":
        w = np.where(at == length - 1, 5.0, 1.0)
    elif kind == "ties":                                           # the maximum twice: a third into the row and at its end
        w = np.where((at == length // 3) | (at == length - 1), 5.0, 1.0)
    else:
        raise KeyError(kind)
    w = np.asarray(w, np.float32) + np.float32(0.0)
    assert np.all(np.isfinite(w)) and not np.any(np.signbit(w) & (w == 0))
    w.setflags(write=False)
    return w


def transposed_weights(name, w):
    """the weights aligned with csr_out's entries (row u, ascending v)"""
    _, _, src, dst = topo_case(name)
    return np.ascontiguousarray(np.asarray(w)[np.lexsort((dst, src))])


@functools.lru_cache(maxsize=None)
def topo_expected(name, kind=None, reverse=False):
    """the model's (level, dist, parent, (peeled, levels, widest)) on the case, or on its reversed graph"""
    cin, _, src, dst = topo_case(name)
    w = None if kind is None else topo_weights(name, kind)
    got = topo_model(cin.num_rows, dst, src, w) if reverse else topo_model(cin.num_rows, src, dst, w)
    for arr in got[:3]:
        if arr is not None:
            arr.setflags(write=False)
    return got


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_topo"), "libgraphlily_hip.so does not export gl_topo"
    assert len(L.gl_topo.argtypes) == 8
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_topo"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_topo" not in capi.EXPORTS and "gl_topo" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.topo) and callable(M.SpMVModule.topo)
    assert callable(app.TopologicalOrder.run) and callable(app.TopologicalOrder.critical_path)
    assert callable(app.validate_topological) and callable(io.directed_weighted)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void topo(SpMVModule *out, DeviceBuffer level, uint32_t *order = nullptr, const float *weight = nullptr" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    topo_h = open(os.path.join(ROOT, "include", "graphlily", "app", "topo.h")).read()
    for piece in ("class TopologicalOrder : public app::PatternApp", "prepare(", "run(", "level()", "dist()", "parent()", "order()",
                  "position()", "num_peeled()", "is_dag()", "level_sizes()", "num_levels()", "widest()", "critical_length()",
                  "critical_path()", "launches()", "util_directed_weighted"):
        assert piece in topo_h
    assert "util_directed_weighted" in open(os.path.join(ROOT, "include", "graphlily", "io", "data_formatter.h")).read()
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_topo.hip" in make and HEADER in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "topo_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_topo(None, None, None, None, None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


def _f64_longest(n, src, dst, w, level):
    """the longest path to every vertex in f64, a DP over the vertices in level order (exact for small integers)"""
    best = np.zeros(n)
    preds = [[] for _ in range(n)]
    for u, v, x in zip(src.tolist(), dst.tolist(), w.tolist()):
        preds[v].append((u, x))
    for v in np.argsort(level, kind="stable").tolist():
        if preds[v]:
            best[v] = max(best[u] + x for u, x in preds[v])
    return best


@pytest.mark.parametrize("name", ACYCLIC)
def test_model_equals_networkx_on_every_acyclic_case(name):
    import networkx as nx
    cin, _, src, dst = topo_case(name)
    n = cin.num_rows
    level, _, _, (peeled, levels, widest) = topo_expected(name)
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(src.tolist(), dst.tolist()))
    gens = [set(g) for g in nx.topological_generations(G)]
    assert peeled == n and levels == len(gens) and widest == max(len(g) for g in gens)
    for k, g in enumerate(gens):
        assert set(np.flatnonzero(level == k).tolist()) == g, k
    assert app.validate_topological(cin, level) == n
    # non-negative integer weights: networkx's longest path; signed ones: an f64 DP (both exact in f32)
    rng = np.random.default_rng(9)
    for lo in (0, -3):
        w = rng.integers(lo, 6, src.shape[0]).astype(np.float32)
        lev, dist, parent, _ = topo_model(n, src, dst, w)
        assert np.array_equal(lev, level)
        if lo == 0:
            G = nx.DiGraph()
            G.add_nodes_from(range(n))
            G.add_weighted_edges_from(zip(src.tolist(), dst.tolist(), w.tolist()))
            assert float(dist.max()) == nx.dag_longest_path_length(G)
        assert np.array_equal(dist.astype(np.float64), _f64_longest(n, src, dst, w, level))
        fed = parent != NONE
        assert np.array_equal(fed, np.bincount(dst, minlength=n) > 0)
        col = {(u, v): x for u, v, x in zip(src.tolist(), dst.tolist(), w.tolist())}
        for v in np.flatnonzero(fed).tolist():                     # the parent attains dist, and no smaller predecessor does
            u = int(parent[v])
            assert dist[u] + col[(u, v)] == dist[v]
            assert all(dist[x] + col[(x, v)] < dist[v] for x in src[dst == v].tolist() if x < u)
        assert app.validate_topological(_csr(n, dst, src, w), lev, dist, parent, weighted=True) == n


def test_closed_forms_of_the_model():
    level, _, _, stats = topo_expected("path_600")
    assert np.array_equal(level[:600], np.arange(600)) and np.all(level[600:] == 0) and stats == (640, 600, 41)
    level, _, _, stats = topo_expected("path_desc_600")
    assert np.array_equal(level[:600], np.arange(600)[::-1]) and stats == (640, 600, 41)
    cin, cout, _, _ = topo_case("tournament_70")
    level, dist, parent, stats = topo_expected("tournament_70", "equal")
    assert np.array_equal(level[:70], np.arange(70)) and stats == (96, 70, 27)
    assert np.array_equal(dist[:70], np.arange(70)) and np.array_equal(parent[1:70], np.arange(69)) and parent[0] == NONE
    assert sorted(np.diff(cin.adj_indptr.astype(np.int64))[:70].tolist()) == list(range(70)) == sorted(np.diff(cout.adj_indptr.astype(np.int64))[:70].tolist())
    assert topo_expected("in_hub_1000")[3] == (1024, 2, 1023) and topo_expected("out_hub_1000")[3] == (1024, 2, 1000)
    cin = topo_case("fan_lengths")[0]
    assert np.diff(cin.adj_indptr.astype(np.int64))[520:532].tolist() == list(FAN_LENGTHS)
    level, dist, parent, stats = topo_expected("fan_lengths", "ties")
    assert stats == (540, 2, 528)
    ip = cin.adj_indptr.astype(np.int64)
    for i, k in enumerate(FAN_LENGTHS):                             # the first of the two maxima wins; a row of 513: step 0 against step 2
        assert dist[520 + i] == 5 and parent[520 + i] == cin.adj_indices[ip[520 + i] + (k // 3 if k > 1 else 0)]
    for kind, at in (("peak_first", 0), ("peak_last", -1), ("equal", 0)):
        _, dist, parent, _ = topo_expected("fan_lengths", kind)
        for i, k in enumerate(FAN_LENGTHS):
            assert parent[520 + i] == cin.adj_indices[ip[520 + i] + (at % k)], (kind, k)
    level = topo_expected("grid_24x24")[0]
    i, j = np.divmod(np.arange(576), 24)
    assert np.array_equal(level, i + j) and topo_expected("grid_24x24")[3] == (576, 47, 24)
    level = topo_expected("tree_1023")[0]
    assert np.array_equal(level, np.floor(np.log2(np.arange(1023) + 1))) and topo_expected("tree_1023")[3] == (1023, 10, 512)
    assert np.all(topo_expected("cycle_5")[0] == NONE) and topo_expected("cycle_5")[3] == (0, 0, 0)
    level, dist, parent, stats = topo_expected("lollipop", "equal")
    assert np.array_equal(level[:10], np.arange(10)) and np.all(level[10:] == NONE) and stats == (10, 10, 1)
    assert np.all(bits(dist[10:]) == NAN_BITS) and np.all(parent[10:] == NONE) and np.array_equal(dist[:10], np.arange(10))
    level = topo_expected("symmetric")[0]
    assert np.all(level[:3] == NONE) and np.all(level[3:] == 0)
    assert topo_expected("empty")[3] == (64, 1, 64)
    # overflow stays deterministic: +inf along the path from the 12th edge on, -inf under negative weights, and never a NaN
    _, dist, _, _ = topo_expected("path_600", "huge_pos")
    assert np.isfinite(dist[11]) and np.all(np.isposinf(dist[12:600]))
    _, dist, _, _ = topo_expected("path_600", "huge_neg")
    assert np.all(np.isneginf(dist[12:600]))
    for name in ACYCLIC:
        for kind in ("huge", "subnormal"):
            d = topo_expected(name, kind)[1]
            assert not np.any(np.isnan(d)) and not np.any(np.signbit(d) & (d == 0)), (name, kind)
    d = topo_expected("path_600", "subnormal")[1]
    assert 0 < d[599] < 1.2e-38 * 600                               # sums of subnormals are kept, not flushed


@pytest.mark.parametrize("name", CYCLIC)
def test_cyclic_cases_peel_what_is_not_behind_a_cycle(name):
    cin, _, src, dst = topo_case(name)
    n = cin.num_rows
    level, dist, parent, (peeled, levels, widest) = topo_expected(name, "signed")
    assert peeled < n and peeled == np.count_nonzero(level != NONE)
    # behind a cycle: reached from a vertex of a non-trivial strongly connected component
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.csr_matrix((np.ones(src.shape[0]), (src, dst)), shape=(n, n))
    _, comp = connected_components(A, directed=True, connection="strong")
    seen = np.bincount(comp)[comp] > 1
    assert np.array_equal(app._reach_inside(src, dst, seen, n), level == NONE)
    assert np.all(bits(dist)[level == NONE] == NAN_BITS) and np.all(parent[level == NONE] == NONE)
    w = topo_weights(name, "signed")
    assert app.validate_topological(_csr(n, dst, src, w), level, dist, parent, weighted=True) == peeled
    rev = topo_expected(name, "signed", True)
    assert np.array_equal(app._topological_of(n, dst, src, w)[0], rev[0])


@pytest.mark.parametrize("name", ["tournament_70_perm", "fan_lengths", "layered_2000_6000_perm", "lollipop", "bowtie", "empty"])
def test_the_numpy_loop_of_the_validator_equals_the_model(name):
    cin, _, src, dst = topo_case(name)
    for kind in (None,) + WEIGHTS:
        w = None if kind is None else topo_weights(name, kind)
        for a, b in ((src, dst), (dst, src)):
            level, dist, parent, _ = topo_expected(name, kind, a is dst)
            got = app._topological_of(cin.num_rows, a, b, w)
            assert np.array_equal(got[0], level), kind
            if kind is not None:
                assert np.array_equal(bits(got[1]), bits(dist)) and np.array_equal(got[2], parent), kind


def test_directed_weighted_keeps_every_rule():
    # 6 vertices: 0 -> 1 stored twice (2.5 and 4), 1 -> 2 with a stored 0, 2 -> 3 with -0.0, a loop at 3 holding a NaN, 3 -> 4 = -7
    rows = [1, 1, 2, 3, 3, 4, 0]
    cols = [0, 0, 1, 2, 3, 3, 5]
    data = [2.5, 4.0, 0.0, -0.0, np.nan, -7.0, 1e-40]
    m = _csr(6, rows, cols, data)
    cin, cout, symmetric = io.directed_weighted(m)
    assert not symmetric and (cin.num_rows, cin.num_cols, cout.num_rows) == (6, 6, 6)
    assert cin.adj_indptr.tolist() == [0, 1, 2, 3, 4, 5, 5] and cin.adj_indices.tolist() == [5, 0, 1, 2, 3]
    assert np.array_equal(bits(cin.adj_data), bits(np.array([1e-40, 4.0, 0.0, 0.0, -7.0])))       # the largest; +0.0; the subnormal kept
    assert cout.adj_indptr.tolist() == [0, 1, 2, 3, 4, 4, 5] and cout.adj_indices.tolist() == [1, 2, 3, 4, 0]
    assert np.array_equal(bits(cout.adj_data), bits(np.array([4.0, 0.0, 0.0, -7.0, 1e-40])))
    for value in (np.nan, np.inf, -np.inf):
        bad = _csr(6, rows, cols, [2.5, 4.0, value, 1.0, np.nan, -7.0, 1.0])
        with pytest.raises(ValueError, match=r"directed_weighted: entry 3 \(2, 1\) is %s" % str(np.float32(value)).replace("+", "")):
            io.directed_weighted(bad)
    # unsorted rows are sorted, a wider matrix is squared, the pattern's symmetry is reported and csr_out still carries ITS weights
    two = io.CSRMatrix(2, 3, [3.0, 1.0, 2.0], [2, 1, 0], [0, 2, 3])
    cin, cout, symmetric = io.directed_weighted(two)
    assert cin.num_rows == 3 and cin.adj_indices.tolist() == [1, 2, 0] and cin.adj_data.tolist() == [1.0, 3.0, 2.0] and not symmetric
    sym = _csr(3, [0, 1, 1, 2], [1, 0, 2, 1], [1.0, 2.0, 3.0, 4.0])
    cin, cout, symmetric = io.directed_weighted(sym)
    assert symmetric and np.array_equal(cin.adj_indices, cout.adj_indices) and cout.adj_data.tolist() == [2.0, 1.0, 4.0, 3.0]
    # weighted=False is simple_pattern, to the bit
    for m in (_csr(6, rows, cols, data), sym, topo_case("bowtie")[0], permute_rows(topo_case("layered_2000_6000_perm")[0], 3)):
        a, b = io.directed_weighted(m, weighted=False), io.simple_pattern(m)
        assert a[2] == b[2] and (a[1] is None) == (b[1] is None)
        for x, y in zip(a[:2], b[:2]):
            if x is not None:
                assert (x.num_rows, x.num_cols) == (y.num_rows, y.num_cols)
                for f in ("adj_indptr", "adj_indices", "adj_data"):
                    assert getattr(x, f).dtype == getattr(y, f).dtype and np.array_equal(getattr(x, f), getattr(y, f))


def test_validate_topological_accepts_the_truth_and_refuses_one_violation_per_rule():
    cin, _, src, dst = topo_case("lollipop")
    w = topo_weights("lollipop", "fractions")
    m = _csr(30, dst, src, w)
    level, dist, parent, (peeled, _, _) = topo_expected("lollipop", "fractions")
    assert app.validate_topological(cin, level) == 10 == peeled
    assert app.validate_topological(m, level, dist, parent, weighted=True) == 10
    pad = lambda a, fill: np.concatenate([a, np.full(98, fill, a.dtype)])
    assert app.validate_topological(m, pad(level, 0), pad(dist, 0), pad(parent, NONE), weighted=True) == 108
    with pytest.raises(ValueError, match="7 levels for a 30 x 30 matrix"):
        app.validate_topological(cin, level[:7])
    with pytest.raises(ValueError, match="needs dist and parent"):
        app.validate_topological(m, level, weighted=True)
    bad = level.copy()
    bad[5] = 3                                                      # 4 -> 5 no longer raises the level
    with pytest.raises(ValueError, match=r"the edge 4 -> 5 goes from level 4 to level 3 \(rule 1\)"):
        app.validate_topological(cin, bad)
    bad = level.copy()
    bad[20] = 11                                                    # peeled behind the cycle
    with pytest.raises(ValueError, match=r"the edge 19 -> 20 goes from level none to level 11 \(rule 1\)"):
        app.validate_topological(cin, bad)
    bad = level.copy()
    bad[6:10] += 1                                                  # a gap: 5 -> 6 rises by two
    with pytest.raises(ValueError, match=r"vertex 6 has level 7 and a predecessor one level below is missing \(rule 2\)"):
        app.validate_topological(cin, bad)
    bad = level.copy()
    bad[:10] += 1                                                   # the source is not at level 0
    with pytest.raises(ValueError, match=r"vertex 0 has level 1 and no predecessor \(rule 2\)"):
        app.validate_topological(cin, bad)
    bad = level.copy()
    bad[9] = NONE                                                   # the end of the first tail left unpeeled
    with pytest.raises(ValueError, match=r"vertex 9 is not peeled and has no unpeeled predecessor \(rule 3\)"):
        app.validate_topological(cin, bad)
    # rule 4 alone: a wrong distance, a parent that is not the smallest
    bad = dist.copy()
    bad[3] = np.nextafter(bad[3], np.float32(9))
    with pytest.raises(ValueError, match=r"vertex 3 has dist .* \(rule 4\)"):
        app.validate_topological(m, level, bad, parent, weighted=True)
    _, _, tsrc, tdst = topo_case("grid_24x24")
    tl, td, tp, _ = topo_expected("grid_24x24", "equal")
    tm = _csr(576, tdst, tsrc, topo_weights("grid_24x24", "equal"))
    assert app.validate_topological(tm, tl, td, tp, weighted=True) == 576
    bad = tp.copy()
    assert td[25] == 2 and td[1] == td[24] == 1 and tp[25] == 1       # both predecessors of (1, 1) attain its distance
    bad[25] = 24
    with pytest.raises(ValueError, match=r"vertex 25 has parent 24, the host loop gives 1 \(rule 4\)"):
        app.validate_topological(tm, tl, td, bad, weighted=True)


def _golden_model(golden_dir):
    raw = io.load_csr_matrix_from_float_npz(os.path.join(golden_dir, GOLDEN))
    cin, cout, sym = io.directed_weighted(raw)
    dst = np.repeat(np.arange(cin.num_rows, dtype=np.int64), np.diff(cin.adj_indptr.astype(np.int64)))
    return raw, cin, cout, topo_model(cin.num_rows, cin.adj_indices.astype(np.int64), dst, cin.adj_data)


def test_golden_fixture_is_the_models(golden_dir):
    """tests/golden/topo_layered_csr_float32.npz: 150 vertices under a seeded permutation -- a layered DAG of 120 (7 levels, every edge
    to a later layer), a cycle of 6 fed from it and a tail of 24 behind the cycle --, weights that are multiples of 0.25 in [-2, 4],
    one edge stored twice, a loop, a stored zero and rows stored unsorted; the expected arrays were made by topo_model"""
    raw, cin, cout, (level, dist, parent, stats) = _golden_model(golden_dir)
    want = np.load(os.path.join(golden_dir, EXPECTED))
    assert (raw.num_rows, raw.num_cols) == (150, 150) and cin.nnz == raw.nnz - 2
    assert np.array_equal(want["topo_level"], level) and np.array_equal(want["topo_dist_bits"], bits(dist)) and np.array_equal(want["topo_parent"], parent)
    assert tuple(want["topo_stats"].tolist()) == stats and stats[0] == 120 and np.count_nonzero(level == NONE) == 30
    assert app.validate_topological(raw, level, dist, parent, weighted=True) == 120


def test_driver_prepares_both_patterns_and_refuses_what_it_cannot_do(golden_dir):
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_topo decrements the counter of every column"):
        app.TopologicalOrder(comm=TwoRanks(), backend=CpuBackend())
    d = app.TopologicalOrder(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (d.n_, d.n_real_) == (128, 8) and d.graph_.nnz == 7 and not d.symmetric_ and d.out_ is not None and not d.weighted_
    assert d.graph_out_.nnz == 7 and len(d.modules_) == 2
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    with pytest.raises(RuntimeError, match="weighted load first"):
        d.critical_path()
    d.load_and_format_matrix(os.path.join(golden_dir, GOLDEN), weighted=True)
    raw, cin, cout, _ = _golden_model(golden_dir)
    assert (d.n_, d.n_real_, d.weighted_) == (256, 150, True) and d.graph_.nnz == cin.nnz == d.graph_out_.nnz
    assert np.array_equal(d.graph_.adj_data[:cin.nnz], cin.adj_data) and np.array_equal(d.graph_out_.adj_indices, cout.adj_indices)
    assert np.all(d.SpMV_.csr.adj_data == 1) and np.all(d.out_.csr.adj_data == 1)      # (the plans are built from ones)
    assert d.SpMV_.csr.nnz == d.out_.csr.nnz == cin.nnz
    cin = topo_case("symmetric")[0]
    d.load_and_format_matrix(cin.copy())                               # a CSRMatrix goes straight in
    assert d.symmetric_ and d.out_ is None and d.graph_out_ is None and len(d.modules_) == 1 and d.n_ == 128
    d.load_and_format_matrix(cin.copy(), weighted=True)                # ... weighted: the transposed weights are kept
    assert d.symmetric_ and d.out_ is None and d.graph_out_ is not None
    for value in (np.nan, np.inf, -np.inf):
        bad = _csr(10, [1, 2], [0, 1], [1.0, value])
        with pytest.raises(ValueError, match=r"directed_weighted: entry 1 \(2, 1\) is"):
            d.load_and_format_matrix(bad, weighted=True)
        d.load_and_format_matrix(bad, weighted=False)                  # (the pattern alone takes any non-zero value)


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("topo_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([TOPO_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
