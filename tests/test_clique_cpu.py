"""The host side of k-clique counting (gl_clique_count, io.orient_by_rank, app.validate_cliques): clique_model -- the formula of
include/graphlily_hip_clique.h as a plain recursion over Python sets and ints, the truth tests/test_gpu_clique.py compares the
kernels with -- against networkx and the closed forms of K_n, the orientation by a caller's rank, and the extension's header
against its own capi.EXT_HEADERS entry and the library."""
import functools
import math
import os
import re

import networkx as nx
import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver
from test_kcore_cpu import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIQUE_DRIVER = os.path.join(ROOT, "build", "clique_driver")
HEADER = "graphlily_hip_clique.h"
DECL = ("int gl_clique_count(gl_spmv_plan plan, uint32_t k, uint64_t *d_total, uint64_t *d_per_vertex /* may be NULL: n words */, "
        "uint64_t *h_stats /* may be NULL: 4 HOST words: rows per bin {tiny+mid, wide, long}, launches */);")
GOLDEN = "similarity_caves_csr_float32.npz"


def clique_model(csr, k):
    """-> (total, per uint64[num_rows]): the sequences (v1 .. vk) with vj in N+(vi) for every i < j, N+(x) = the set of row x;
    per[x] = the positions x holds in them.  No orientation is assumed: a symmetric pattern gives k! times the cliques."""
    ip = csr.adj_indptr.astype(np.int64)
    rows = [frozenset(int(u) for u in csr.adj_indices[ip[v]:ip[v + 1]]) for v in range(csr.num_rows)]
    per = [0] * csr.num_rows
    total = 0

    def descend(prefix, cand):
        nonlocal total
        if len(prefix) == k - 1:
            total += len(cand)
            for u in cand:
                per[u] += 1
            for u in prefix:
                per[u] += len(cand)
            return
        for u in cand:
            descend(prefix + [u], cand & rows[u])

    for v in range(csr.num_rows):
        descend([v], rows[v])
    return total % 2 ** 64, np.array([c % 2 ** 64 for c in per], dtype=np.uint64)


def graph_csr(g):
    """a networkx graph over 0 .. n - 1 as a CSR with both directions of every edge"""
    e = np.array(list(g.edges()), dtype=np.int64).reshape(-1, 2)
    return _csr(g.number_of_nodes(), np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))


def complete_oriented(n):
    rows, cols = np.triu_indices(n, 1)
    return _csr(n, rows, cols)


@functools.lru_cache(maxsize=None)
def row_case(d, seed=5):
    """-> (oriented csr, rank): vertex 0 is joined to the d vertices 1 .. d and a rank that only ties makes it the source of a row
    of exactly d entries; the local graph on 1 .. d is sparse -- 3 d random pairs -- with three planted cliques of min(7, d)
    vertices, so that every k up to 8 finds something where d allows it."""
    rng = np.random.default_rng(seed + d)
    local = [rng.integers(1, d + 1, size=(3 * d, 2))]
    for _ in range(3):
        c = rng.choice(np.arange(1, d + 1), size=min(7, d), replace=False)
        local.append(np.array([(a, b) for a in c for b in c if a < b], dtype=np.int64).reshape(-1, 2))
    e = np.concatenate(local + [np.stack([np.zeros(d, np.int64), np.arange(1, d + 1)], axis=1)])
    rank = np.ones(d + 1, dtype=np.uint32)
    rank[0] = 0
    csr, _ = io.orient_by_rank(_csr(d + 1, e[:, 0], e[:, 1]), rank)
    assert int(csr.adj_indptr[1]) == d
    for arr in (csr.adj_indptr, csr.adj_indices, csr.adj_data):
        arr.setflags(write=False)
    return csr, rank


NX_CASES = {"karate": nx.karate_club_graph, "caveman": lambda: nx.connected_caveman_graph(4, 6), "k7": lambda: nx.complete_graph(7),
            "gnp": lambda: nx.gnp_random_graph(30, 0.4, seed=3), "petersen": nx.petersen_graph}


@pytest.mark.parametrize("name", sorted(NX_CASES))
def test_model_equals_networkx_and_the_symmetric_pattern_counts_every_order(name):
    g = nx.convert_node_labels_to_integers(NX_CASES[name]())
    sym = graph_csr(g)
    oriented, deg = io.orient_by_rank(sym)
    assert deg.tolist() == [g.degree(v) for v in range(g.number_of_nodes())]
    for k in range(3, 7):
        cliques = [c for c in nx.enumerate_all_cliques(g) if len(c) == k]
        want = np.bincount(np.array(cliques, dtype=np.int64).ravel(), minlength=oriented.num_rows)
        total, per = clique_model(oriented, k)
        assert total == len(cliques) and np.array_equal(per, want.astype(np.uint64)), (name, k)
        assert app.validate_cliques(sym, k, per) == total
        if k <= 4:
            total_sym, per_sym = clique_model(sym, k)
            assert total_sym == math.factorial(k) * total and np.array_equal(per_sym, math.factorial(k) * per), (name, k)
    if g.number_of_edges() and per.shape[0]:
        wrong = clique_model(oriented, 3)[1]
        wrong[int(np.argmax(wrong))] += 1
        with pytest.raises(ValueError, match="validate_cliques: vertex"):
            app.validate_cliques(sym, 3, wrong)


@pytest.mark.parametrize("n", [4, 9, 33])
def test_model_closed_forms_of_complete_graphs(n):
    for k in range(3, 7):
        total, per = clique_model(complete_oriented(n), k)
        assert total == math.comb(n, k) and per.tolist() == [math.comb(n - 1, k - 1)] * n, (n, k)


def test_model_diagonal_entry_takes_part_and_short_rows_give_nothing():
    # 0 -> {0, 1, 2}, 1 -> {2}: the sequences (0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 2): a vertex is credited per position
    total, per = clique_model(_csr(3, [0, 0, 0, 1], [0, 1, 2, 2]), 3)
    assert total == 4 and per.tolist() == [8, 2, 2]
    # a row of ONE entry is not too short where that entry is on a diagonal: 0 -> {1}, 1 -> {1} gives (0, 1, 1, ...) for every k
    assert [clique_model(_csr(2, [0, 1], [1, 1]), k)[0] for k in (3, 4, 5)] == [2, 2, 2]
    assert clique_model(row_case(3)[0], 6)[0] == 0


@pytest.mark.parametrize("seed", range(4))
def test_orient_by_rank_without_a_rank_is_triangle_orient(seed):
    rng = np.random.default_rng(seed)
    n, m = 60, 400
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)             # duplicates, the diagonal, zero values, both directions
    raw = _csr(n, rows, cols, data=rng.integers(0, 3, m).astype(np.float32))
    got, deg = io.orient_by_rank(raw)
    want, want_deg = io.triangle_orient(raw)
    for a, b in ((got.adj_indptr, want.adj_indptr), (got.adj_indices, want.adj_indices), (got.adj_data, want.adj_data), (deg, want_deg)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert (got.num_rows, got.num_cols) == (want.num_rows, want.num_cols)


@pytest.mark.parametrize("seed", range(3))
def test_orient_by_rank_honours_the_rank_and_breaks_ties_by_vertex(seed):
    rng = np.random.default_rng(10 + seed)
    n, m = 40, 300
    raw = _csr(n, rng.integers(0, n, m), rng.integers(0, n, m))
    rank = rng.integers(0, 4, n).astype(np.uint32)                        # four values over forty vertices: mostly ties
    got, deg = io.orient_by_rank(raw, rank)
    sym, sym_deg = io.symmetrize_simple(raw)
    assert np.array_equal(deg, sym_deg)
    ip, sp = got.adj_indptr.astype(np.int64), sym.adj_indptr.astype(np.int64)
    for v in range(n):
        want = [int(u) for u in sym.adj_indices[sp[v]:sp[v + 1]] if (rank[u], u) > (rank[v], v)]
        assert got.adj_indices[ip[v]:ip[v + 1]].tolist() == want, v
    assert clique_model(got, 3)[0] == clique_model(io.triangle_orient(raw)[0], 3)[0]      # any acyclic orientation: every clique once
    for bad in (rank[:-1], rank.astype(np.int64), rank.astype(np.float32)):
        with pytest.raises(ValueError, match="orient_by_rank"):
            io.orient_by_rank(raw, bad)


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_clique_count"), "libgraphlily_hip.so does not export gl_clique_count"
    assert len(L.gl_clique_count.argtypes) == 5
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert DECL in raw and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))) == capi.EXT_HEADERS[HEADER] == ["gl_clique_count"]
    assert "gl_clique_count" not in capi.EXPORTS and "gl_clique_count" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.clique_count) and callable(M.SpMVModule.clique_count)
    assert callable(app.CliqueCount.run) and callable(app.CliqueCount.clique_density) and callable(app.validate_cliques)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void clique_count(uint32_t k, DeviceBuffer total, uint64_t *per_vertex = nullptr, uint64_t *stats = nullptr)" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_clique.hip" in make and HEADER in make
    assert "clique_driver.cpp" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    if capi.device_count() == 0:
        assert L.gl_clique_count(None, 3, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


def test_cpp_driver_compiles_without_warnings():
    assert build_cpp_driver("clique_driver.cpp") == CLIQUE_DRIVER
