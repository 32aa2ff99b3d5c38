"""CPU side of delta-stepping shortest paths (gl_sssp_delta): io.directed_weighted's keep=, the host validator against results
written out by hand and against scipy's f64 Dijkstra, and this extension's own header against capi.EXT_HEADERS and the library."""
import os
import re

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "graphlily_hip_sssp_delta.h"


@pytest.mark.parametrize("keep,want", [(None, [7, 5]), ("largest", [7, 5]), ("smallest", [2, 5])])
def test_directed_weighted_keeps_the_asked_value_of_parallel_edges(keep, want):
    """row 1 stores the edge 0 -> 1 three times (2, 7, 3) and 2 -> 1 once; the default stays the largest"""
    m = io.CSRMatrix(3, 3, np.array([2, 7, 3, 5], np.float32), np.array([0, 0, 0, 2], np.uint32), np.array([0, 0, 4, 4], np.uint32))
    g_in, g_out, symmetric = io.directed_weighted(m) if keep is None else io.directed_weighted(m, True, keep)
    assert g_in.adj_data.tolist() == want and g_in.adj_indices.tolist() == [0, 2] and not symmetric
    assert g_out.adj_data.tolist() == want and g_out.adj_indptr.tolist() == [0, 1, 1, 2]
    with pytest.raises(ValueError, match="keep"):
        io.directed_weighted(m, True, "first")


@pytest.mark.parametrize("what", ["truth", "too_short", "too_long", "parent_not_smallest"])
def test_validate_shortest_paths(what):
    """0 -> 1 -> 3 and 0 -> 2 -> 3, both of length 2: vertex 3 has two predecessors that fit, and 1 is the smaller"""
    m = io.CSRMatrix(5, 5, np.ones(4, np.float32), np.array([0, 0, 1, 2], np.uint32), np.array([0, 0, 1, 2, 4, 4], np.uint32))
    dist, parent = np.array([0, 1, 1, 2, np.inf], np.float32), np.array([0, 0, 0, 1, 0xFFFFFFFF], np.uint32)
    if what == "truth":
        assert app.validate_shortest_paths(m, 0, dist, parent) == 4 and app.validate_shortest_paths(m, [0], dist) == 4
        return
    if what == "parent_not_smallest":
        parent[3] = 2
    else:
        dist[3] = np.float32(1.5 if what == "too_short" else 2.5)
    with pytest.raises(ValueError, match="vertex 3 has %s" % ("parent 2" if what == "parent_not_smallest" else "distance .* too %s" % what[4:])):
        app.validate_shortest_paths(m, 0, dist, parent)


@pytest.mark.parametrize("symmetric", [False, True])
def test_validate_shortest_paths_accepts_scipys_dijkstra(symmetric):
    """integer weights: sums below 2^24 are exact in f32, so the f64 result, rounded, is the f32 one"""
    import scipy.sparse as sp
    import scipy.sparse.csgraph
    m = datasets.rmat(512, 4096, 9, symmetric=symmetric)
    m = io.CSRMatrix(512, 512, np.random.default_rng(2).integers(1, 256, size=m.nnz).astype(np.float32), m.adj_indices, m.adj_indptr)
    g_in = io.directed_weighted(m, True, "smallest")[0]
    a = sp.csr_matrix((g_in.adj_data.astype(np.float64), g_in.adj_indices, g_in.adj_indptr), shape=(512, 512))
    want = sp.csgraph.dijkstra(a.T.tocsr(), indices=[3, 400], min_only=True)
    assert app.validate_shortest_paths(m, [3, 400], want.astype(np.float32)) == int(np.isfinite(want).sum()) > 100


def test_validate_shortest_paths_on_zero_weights_and_overflow():
    """0 -3e38-> 1 -3e38-> 2 overflows: 2 is unreached and has no parent; 1 -0-> 3 -0-> 1: 3 is an orphan"""
    m = io.CSRMatrix(4, 4, np.array([3e38, 0, 3e38, 0], np.float32), np.array([0, 3, 1, 1], np.uint32), np.array([0, 0, 2, 3, 4], np.uint32))
    dist, parent = np.array([0, 3e38, np.inf, 3e38], np.float32), np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    assert app.validate_shortest_paths(m, 0, dist, parent) == 3


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_sssp_delta") and len(L.gl_sssp_delta.argtypes) == 10
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))) == sorted(capi.EXT_HEADERS[HEADER]) == ["gl_sssp_delta"]
    assert '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert "gl_sssp_delta" not in capi.EXPORTS and "gl_sssp_delta" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.sssp_delta) and callable(M.SpMVModule.sssp_delta)
    assert callable(app.ShortestPaths.run) and callable(app.ShortestPaths.path) and issubclass(app.TopologicalOrder, app._DirectedPairApp)
    if capi.device_count() == 0:
        assert L.gl_sssp_delta(None, None, None, None, None, 0, 1.0, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


def test_walk_stars_one_entry_of_every_hub_row_decides():
    """the inputs of tests/test_gpu_walk.py::test_sssp_delta: without the last entry of every hub row and its mirror the sources
    reach nobody; without the first, the first leaf is unreached -- so a push or a parent pull that loses one end of a long row
    cannot return dijkstra_f32's answer.  (The star whose hub is a source itself keeps its hub; it loses its first leaf.)"""
    from test_gpu_sssp_delta import bits
    from test_gpu_walk import DEGREES, _stars, sssp_stars, star_hubs
    for sources in ("one", "every", "with_a_hub"):
        g, src, (dist, parent, orphans) = sssp_stars(sources)
        hubs = star_hubs(max(DEGREES)) if sources == "one" else star_hubs(1)
        hubs = hubs[~np.isin(hubs, src)]
        last = hubs + np.diff(g.adj_indptr.astype(np.int64))[hubs]
        assert np.array_equal(parent[hubs], last) and np.array_equal(dist[hubs], last - hubs) and orphans == 0
        less = sssp_stars(sources, "last")[2]
        assert np.all(np.isinf(less[0][hubs])) and np.all(less[1][hubs] == 0xFFFFFFFF)
        less = sssp_stars(sources, "first")[2]
        one_leaf = last == hubs + 1
        assert np.all(np.isinf(less[0][hubs + 1][~one_leaf])) and np.all(np.isinf(less[0][hubs][one_leaf])) and np.isfinite(dist[hubs + 1]).all()
        assert np.count_nonzero(bits(less[0]) != bits(dist)) >= hubs.shape[0]
