"""Graph contraction without a GPU: the library exports and binds gl_contract_*, the drivers exist, app.validate_quotient accepts
io.aggregate_communities' own output and rejects a spoiled one, and its directed statement is
StronglyConnectedComponents.condensation()'s matrix.  tests/test_gpu_contract.py runs the kernels."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver
from test_spgemm_cpu import random_csr
from test_tc_cpu import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUOTIENT_DRIVER = os.path.join(ROOT, "build", "quotient_driver")
HEADER = "graphlily_hip_contract.h"


def smallest_member(groups):
    """-> uint32 labels: every vertex labelled with the smallest vertex of its group, gl_cc's convention"""
    return app._smallest_member_labels(np.unique(groups, return_inverse=True)[1].reshape(-1), len(groups))


@functools.lru_cache(maxsize=None)
def directed_graph():
    """a small directed R-MAT: 256 vertices, 1500 draws (duplicates and a few diagonal entries among them)"""
    rng = np.random.default_rng(17)
    rows = cols = np.zeros(1500, np.int64)
    for _ in range(8):
        quad = rng.choice(4, size=1500, p=[0.45, 0.22, 0.22, 0.11])
        rows, cols = 2 * rows + quad // 2, 2 * cols + quad % 2
    key = np.unique(rows * 256 + cols)
    return _csr(256, key // 256, key % 256)


def test_library_exports_and_binds_the_entry_points():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    names = ["gl_contract_numeric", "gl_contract_symbolic"]
    assert capi.EXT_HEADERS[HEADER] == names
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert sorted(set(re.findall(r"^int (gl_\w+)\(", text, re.M))) == names
    for name in names:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    for cls, method in ((capi.SpMVPlan, "contract_symbolic"), (capi.SpMVPlan, "contract_numeric"), (M.SpMVModule, "contract"), (app.QuotientGraph, "run")):
        assert callable(getattr(cls, method))
    assert app.QuotientGraph._no_shards_ and inspect.signature(app.Louvain.run).parameters["aggregate"].default in ("host", "device")
    assert build_cpp_driver("quotient_driver.cpp") == QUOTIENT_DRIVER


@pytest.mark.parametrize("labelling", ["blocks_of_7", "random_40"])
def test_validate_quotient_accepts_the_truth_and_rejects_a_spoiled_result(labelling):
    raw = random_csr(300, 2400, 4)
    sym = io.symmetrize_simple(raw)[0]
    rng = np.random.default_rng(2)
    labels = np.arange(300) // 7 * 7 if labelling == "blocks_of_7" else rng.integers(0, 40, 300)
    weights = rng.integers(1, 1000, sym.nnz).astype(np.uint32)
    c, w, tot, part = io.aggregate_communities(sym, weights, None, labels)
    assert app.validate_quotient(raw, labels, (c, w, tot, part), directed=False, weights=weights) == c.num_rows
    heavier = w.copy()
    heavier[5] += 1
    with pytest.raises(ValueError, match=r"weights\[5\]"):
        app.validate_quotient(raw, labels, (c, heavier, tot, part), directed=False, weights=weights)
    swapped = c.copy()
    swapped.adj_indices[[0, 1]] = swapped.adj_indices[[1, 0]]
    assert c.adj_indptr[1] >= 2
    with pytest.raises(ValueError, match=r"adj_indices\[0\]"):
        app.validate_quotient(raw, labels, (swapped, w, tot, part), directed=False, weights=weights)


def test_directed_statement_is_the_condensation():
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    raw = directed_graph()
    n = raw.num_rows
    graph = io.simple_pattern(raw)[0]
    A = sp.csr_matrix((np.ones(graph.nnz), graph.adj_indices, graph.adj_indptr), shape=(n, n))
    labels = smallest_member(csgraph.connected_components(A, directed=True, connection="strong")[1])
    scc = app.StronglyConnectedComponents.__new__(app.StronglyConnectedComponents)      # condensation() reads these fields alone
    scc.graph_, scc.labels_, scc.n_real_ = graph, labels, n
    scc.component_labels_ = np.unique(labels)
    scc.num_components_ = scc.component_labels_.shape[0]
    dag, rank = scc.condensation()
    c, w, tot, part = app._quotient_of(graph, labels, None, None)
    assert 1 < c.num_rows < n and np.array_equal(c.adj_indptr, dag.adj_indptr) and np.array_equal(c.adj_indices, dag.adj_indices)
    assert np.array_equal(part, rank[labels]) and int(w.sum()) <= graph.nnz and int(tot.sum()) == graph.nnz
    assert app.validate_quotient(raw, labels, (c, w, tot, part)) == c.num_rows


@pytest.mark.parametrize("members", [18, 65, 129])
def test_walk_stars_one_entry_of_every_hub_row_decides(members):
    """the inputs of tests/test_gpu_contract.py::test_walk_stars_in_one_group: without the last (first) entry of every hub row and
    its mirror, the product row of the hubs' group loses every such leaf that is not a member itself, and the group's tot the
    weight of all 17 -- so a walk that loses one end of a member row cannot return io.aggregate_communities' answer"""
    from test_gpu_contract import contract_stars
    from test_gpu_walk import _stars, star_hubs
    hubs, last = star_hubs(1), _stars()[4]
    g, labels, weights = contract_stars(members)
    c, w, tot, part = io.aggregate_communities(g, weights, None, labels)
    row = set(c.adj_indices[:c.adj_indptr[1]].tolist())
    assert len(row) == 2519 - (members - 18) and np.count_nonzero(part == 0) == members
    for drop, gone in (("last", last), ("first", hubs + 1)):
        less = contract_stars(members, drop)
        cl, wl, totl, partl = io.aggregate_communities(less[0], less[2], None, less[1])
        assert np.array_equal(partl, part) and less[0].nnz == g.nnz - 2 * 17
        lost = row - set(cl.adj_indices[:cl.adj_indptr[1]].tolist())
        assert lost == set(part[gone][part[gone] != 0].tolist()) and (members > 18 or len(lost) == 17)
        assert tot[0] - totl[0] == sum(int(weights[g.adj_indptr[h]:g.adj_indptr[h + 1]][-1 if drop == "last" else 0]) for h in hubs) + \
            sum(int(weights[g.adj_indptr[v]]) for v in gone if part[v] == 0)
