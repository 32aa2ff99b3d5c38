"""CPU suite of the k-truss decomposition (gl_truss, SpMVPlan.truss, SpMVModule.truss, app.KTruss, app.validate_truss): the export
and its bindings exist, the host-side validator accepts networkx's truss numbers and refuses one violation per rule, its set peel
agrees with a one-edge-at-a-time statement of the definition and with closed forms, the driver refuses what it cannot do, and the
C++ driver compiles against include/.  tests/test_gpu_truss.py compares the kernels with truss_numbers (kept here) bit for bit."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver, named_matrix
from test_tc_cpu import GRAPHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUSS_DRIVER = os.path.join(ROOT, "build", "truss_driver")
HEADER = "graphlily_hip_truss.h"
DECL = "int gl_truss(gl_spmv_plan plan, uint32_t *d_truss, uint32_t *d_support /* may be NULL */, uint64_t *h_stats /* may be NULL, 6 words */);"
# (max truss, sum of truss over the edges, triangles, sub-rounds) of the graphs padded to 128.  Two methods agree on every line: the
# validator's set peel over the triangle list (app._truss_numbers_of) and, on the graphs of test_tc_cpu.GRAPHS, a host replay of
# the device's schedule a whole launch at a time with the edges of a slice in random order; networkx.k_truss (3.4.2) for every k
# gave the same truss numbers on uniform, rmat_sym, messy and many, and test_validate_truss_accepts_networkx recomputes three of
# them with networkx every time.  The triangles equal test_tc_cpu's counts.
RECORDS = {
    "uniform": (3, 36716, 256, 3),
    "rmat": (27, 248922, 132128, 165),
    "rmat_sym": (19, 128650, 63060, 123),
    "messy": (4, 58422, 2839, 5),
    "many": (3, 181579, 1, 2),
    "rmat_20K": (91, 9484925, 6312502, 1132),
}
LEVELS = {"uniform": 2, "rmat": 26, "rmat_sym": 18, "messy": 3, "many": 2, "rmat_20K": 90}


def _csr(n, rows, cols):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return io.CSRMatrix(n, n, np.ones(rows.shape[0], np.float32), cols.astype(np.uint32), np.cumsum(indptr).astype(np.uint32))


def graph_of(n, a, b):
    """the undirected simple graph with the edges {a[i], b[i]} on n vertices, as gl_truss wants it"""
    return io.symmetrize_simple(_csr(n, a, b))[0]


def entry_rows(sym):
    return np.repeat(np.arange(sym.num_rows, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))


def truss_by_single_edges(sym):
    """The definition, one edge at a time: repeatedly remove an edge that lies in the fewest remaining triangles; truss - 2 = the
    largest such count seen up to the edge's removal.  -> uint32[nnz], one value per entry.  Sets of neighbours, no triangle list,
    no levels: nothing in common with the validator's peel but the definition."""
    import heapq
    n = sym.num_rows
    ip, idx = sym.adj_indptr.astype(np.int64).tolist(), sym.adj_indices.astype(np.int64).tolist()
    nb = [set(idx[ip[v]:ip[v + 1]]) - {v} for v in range(n)]
    sup = {(u, v): len(nb[u] & nb[v]) for u in range(n) for v in nb[u] if u < v}
    heap = [(s, e) for e, s in sup.items()]
    heapq.heapify(heap)
    out, k = {}, 0
    while heap:
        s, e = heapq.heappop(heap)
        if e in out or s != sup[e]:
            continue
        k = max(k, s)
        out[e] = k + 2
        u, v = e
        for w in nb[u] & nb[v]:
            for f in ((min(u, w), max(u, w)), (min(v, w), max(v, w))):
                sup[f] -= 1
                heapq.heappush(heap, (sup[f], f))
        nb[u].discard(v)
        nb[v].discard(u)
    rows = entry_rows(sym).tolist()
    return np.array([out[(min(r, c), max(r, c))] if r != c else 0 for r, c in zip(rows, idx)], dtype=np.uint32)


def truss_numbers(sym):
    """-> (truss as uint32[nnz], support as uint32[nnz], levels, sub_rounds, triangles) by the validator's set peel"""
    eid, eu, ev, tri = app._edges_and_triangles_of(sym.adj_indptr, sym.adj_indices, sym.num_rows)
    truss, support, levels, sub_rounds = app._truss_numbers_of(eu.shape[0], tri)
    on = eid >= 0
    return (np.where(on, truss[eid], 0).astype(np.uint32), np.where(on, support[eid], 0).astype(np.uint32), levels, sub_rounds,
            tri.shape[0])


def summary(sym, truss, sub_rounds, triangles):
    once = sym.adj_indices.astype(np.int64) > entry_rows(sym)
    return int(truss.max()) if truss.size else 0, int(truss[once].astype(np.int64).sum()), triangles, sub_rounds


@functools.lru_cache(maxsize=None)
def prepared(name):
    """-> (the matrix as given, padded to 128, its symmetric simple form, truss and support per entry of that form, levels,
    sub-rounds); computed once and shared, never written"""
    raw = GRAPHS[name]() if name in GRAPHS else named_matrix(name)
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    sym, _ = io.symmetrize_simple(m)
    truss, support, levels, sub_rounds, triangles = truss_numbers(sym)
    truss.setflags(write=False)
    support.setflags(write=False)
    assert summary(sym, truss, sub_rounds, triangles) == RECORDS[name] and levels == LEVELS[name]
    return raw, m, sym, truss, support, levels, sub_rounds


def _nx_truss(sym):
    """networkx.k_truss for every k -> uint32[nnz]"""
    import networkx as nx
    rows, cols = entry_rows(sym).tolist(), sym.adj_indices.tolist()
    G = nx.Graph()
    G.add_edges_from(zip(rows, cols))
    of, k = {}, 2
    while G.number_of_edges():
        G = nx.k_truss(G, k)
        for u, v in G.edges():
            of[(min(u, v), max(u, v))] = k
        k += 1
    return np.array([of[(min(r, c), max(r, c))] for r, c in zip(rows, cols)], dtype=np.uint32)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_truss"), "libgraphlily_hip.so does not export gl_truss"
    assert len(L.gl_truss.argtypes) == 4
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_truss"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_truss" not in capi.EXPORTS and "gl_truss" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.truss) and callable(M.SpMVModule.truss)
    assert callable(app.KTruss.run) and callable(app.KTruss.k_truss) and callable(app.validate_truss)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "truss(DeviceBuffer truss, uint32_t *support = nullptr, uint64_t *stats = nullptr)" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    truss_h = open(os.path.join(ROOT, "include", "graphlily", "app", "truss.h")).read()
    for piece in ("class KTruss", "run(bool want_support = false)", "max_truss()", "truss_sizes()", "vertex_truss()", "util_symmetrize_simple"):
        assert piece in truss_h
    assert "gl_truss.hip" in open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "truss_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_truss(None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


def _clique_edges(k, first=0):
    iu = np.triu_indices(k, 1)
    return iu[0] + first, iu[1] + first


def book_on_a_clique(p, n):
    """K_5 on 0 .. 4 whose edge (0, 1) is also the spine of p triangles (0, 1, 5 + i) -> the graph, and truss and support per entry"""
    a, b = _clique_edges(5)
    pages = np.arange(5, 5 + p)
    g = graph_of(n, np.concatenate([a, np.zeros(p, np.int64), np.ones(p, np.int64)]), np.concatenate([b, pages, pages]))
    rows, cols = entry_rows(g), g.adj_indices.astype(np.int64)
    page = (rows >= 5) | (cols >= 5)
    spine = (np.minimum(rows, cols) == 0) & (np.maximum(rows, cols) == 1)
    return g, np.where(page, 3, 5).astype(np.uint32), np.where(page, 1, np.where(spine, 3 + p, 3)).astype(np.uint32)


def glued_cliques(n):
    """K_6, K_5, K_4, K_3 in a chain, each glued to the next along one edge -> the graph and truss per entry: every edge has the
    truss of the largest clique it lies in"""
    a, b, size_of, first = [], [], {}, 0
    for k in (6, 5, 4, 3):
        x, y = _clique_edges(k, first)
        for u, v in zip(x.tolist(), y.tolist()):
            size_of[(u, v)] = max(size_of.get((u, v), 0), k)
        a.append(x)
        b.append(y)
        first += k - 2                                                   # the last two vertices are the next clique's first two
    g = graph_of(n, np.concatenate(a), np.concatenate(b))
    rows, cols = entry_rows(g).tolist(), g.adj_indices.tolist()
    return g, np.array([size_of[(min(r, c), max(r, c))] for r, c in zip(rows, cols)], dtype=np.uint32)


def test_single_edge_definition_set_peel_and_closed_forms_agree():
    for g, want, support in (book_on_a_clique(1, 128), book_on_a_clique(7, 128)):
        assert np.array_equal(truss_by_single_edges(g), want)
        got = truss_numbers(g)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], support)
        assert app.validate_truss(g, want) == 5
    g, want = glued_cliques(128)
    assert np.array_equal(truss_by_single_edges(g), want) and np.array_equal(truss_numbers(g)[0], want)
    assert app.validate_truss(g, want) == 6 and sorted(np.unique(want).tolist()) == [3, 4, 5, 6]
    a, b = _clique_edges(17, 3)
    g = graph_of(128, a, b)
    truss, support, levels, sub_rounds, triangles = truss_numbers(g)
    assert np.all(truss == 17) and np.all(support == 15) and (levels, sub_rounds, triangles) == (1, 1, 680)
    rim = np.arange(1, 201)                                              # the wheel: hub 0, 200 rim vertices
    g = graph_of(256, np.concatenate([np.zeros(200, np.int64), rim]), np.concatenate([rim, np.roll(rim, -1)]))
    truss, support, levels, sub_rounds, triangles = truss_numbers(g)
    # (the rim edges lie in one triangle and go first; every spoke is then asked to come down twice, from 2, and stops at 1)
    assert np.all(truss == 3) and triangles == 200 and (levels, sub_rounds) == (1, 2)
    assert np.array_equal(np.unique(support), [1, 2])
    left, right = np.repeat(np.arange(40), 50), np.tile(np.arange(40, 90), 40)            # K_{40,50}: no triangle
    g = graph_of(128, left, right)
    truss, support, levels, sub_rounds, triangles = truss_numbers(g)
    assert np.all(truss == 2) and not support.any() and (levels, sub_rounds, triangles) == (1, 1, 0)
    assert app.validate_truss(g, truss) == 2
    e = _csr(128, [], [])
    assert app.validate_truss(e, np.zeros(0, np.uint32)) == 0


def test_set_peel_agrees_with_the_single_edge_definition_on_messy():
    _, _, sym, truss, _, _, _ = prepared("messy")
    assert np.array_equal(truss_by_single_edges(sym), truss)


@pytest.mark.parametrize("graph", ["uniform", "messy", "many"])
def test_validate_truss_accepts_networkx(graph):
    raw, m, sym, truss, _, _, _ = prepared(graph)
    want = _nx_truss(sym)
    assert np.array_equal(truss, want)
    assert app.validate_truss(m, want) == RECORDS[graph][0]
    assert app.validate_truss(raw, want) == RECORDS[graph][0]          # (the padding adds no entry)
    assert app.validate_truss(sym, want) == RECORDS[graph][0]


@pytest.mark.parametrize("graph", ["rmat", "rmat_sym"])
def test_records_of_the_larger_graphs(graph):
    _, m, sym, truss, support, _, _ = prepared(graph)                    # (prepared asserts RECORDS and LEVELS)
    assert app.validate_truss(m, truss) == RECORDS[graph][0]
    once = sym.adj_indices.astype(np.int64) > entry_rows(sym)
    assert int(support[once].astype(np.int64).sum()) == 3 * RECORDS[graph][2]


def test_validate_truss_refuses_one_violation_per_rule():
    _, m, sym, truss, support, _, _ = prepared("rmat_sym")
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    with pytest.raises(ValueError, match="truss numbers for the %d entries" % sym.nnz):
        app.validate_truss(m, truss[:100])

    def both(j):
        """the entry j and its mirror"""
        ip = sym.adj_indptr.astype(np.int64)
        r, c = int(rows[j]), int(cols[j])
        return [j, int(ip[c] + np.searchsorted(cols[ip[c]:ip[c + 1]], r))]
    # rule 1: the two entries of an edge differ; a value below 2; a value too high
    j = int(np.flatnonzero(truss == truss.max())[0])
    bad = truss.copy()
    bad[max(both(j))] -= 1
    with pytest.raises(ValueError, match=r"entry %d \(%d, %d\) is given truss %d, its mirror entry %d \(rule 1\)"
                       % (max(both(j)), rows[max(both(j))], cols[max(both(j))], truss[j] - 1, truss[j])):
        app.validate_truss(m, bad)
    bad = truss.copy()
    j = int(np.flatnonzero(truss == 2)[0])
    bad[both(j)] = 1
    with pytest.raises(ValueError, match=r"is given truss 1, an edge has at least 2 \(rule 1\)"):
        app.validate_truss(m, bad)
    j = int(np.flatnonzero((truss == truss.max()) & (cols > rows))[0])
    bad = truss.copy()
    bad[both(j)] += 1
    with pytest.raises(ValueError, match=r"entry %d \(%d, %d\) is given truss %d, but only \d+ of its triangles have two other edges that high \(rule 1\)"
                       % (j, rows[j], cols[j], truss[j] + 1)):
        app.validate_truss(m, bad)
    # rule 2: a value too low passes rule 1 (fewer triangles are asked for) and is caught by the independent computation
    bad = np.minimum(truss, truss.max() - 1)                             # (the top class one lower: rule 1 holds everywhere)
    with pytest.raises(ValueError, match=r"entry %d \(%d, %d\) is given truss %d, its truss number is %d \(rule 2\)"
                       % (j, rows[j], cols[j], truss[j] - 1, truss[j])):
        app.validate_truss(m, bad)
    with pytest.raises(ValueError, match=r"rule 2"):
        app.validate_truss(m, np.minimum(truss, 3))                      # (every edge at most 3: rule 1 holds everywhere)


class _TwoRanks:
    """what the drivers ask of a communicator, claiming rank 0 of 2"""
    rank, world_size, distributed = 0, 2, True


def test_driver_refuses_row_shards_and_a_run_before_send(golden_dir):
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_truss reads row u"):
        app.KTruss(comm=_TwoRanks(), backend=CpuBackend())
    kt = app.KTruss(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        kt.run()
    kt.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (kt.n_, kt.n_real_) == (128, 8) and kt.graph_.nnz == 14 and kt.degrees_[:8].max() == 2
    assert np.array_equal(kt.graph_.adj_indices, io.symmetrize_simple(kt.graph_)[0].adj_indices)
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        kt.run(support=True)
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        kt.k_truss(3)


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("truss_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([TRUSS_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
