"""CPU suite of the triangle counting (gl_tc_count, SpMVPlan.tc_count, SpMVModule.tc_count, io.triangle_orient, app.TriangleCount,
app.validate_triangles): the export and its bindings exist, the scipy statement of the definition (kept here; tests/test_gpu_tc.py
compares the kernels with it bit for bit) agrees with networkx on generated graphs, the orientation keeps every triangle exactly
once and makes hub rows short, the host-side validator accepts a correct array and rejects wrong ones, the driver refuses what it
cannot do, and the C++ driver compiles against include/ and fails loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver, named_matrix
from test_cc_cpu import many_components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TC_DRIVER = os.path.join(ROOT, "build", "tc_driver")
DECL = "int gl_tc_count(gl_spmv_plan plan, uint64_t *d_total, uint64_t *d_per_vertex /* may be NULL */);"


def _pattern(m):
    """the stored pattern of a CSRMatrix as a scipy matrix of int64 ones (duplicates would add up: the callers pass sets)"""
    import scipy.sparse as sp
    nnz = m.nnz
    return sp.csr_matrix((np.ones(nnz, np.int64), m.adj_indices[:nnz].astype(np.int64), m.adj_indptr.astype(np.int64)),
                         shape=(m.num_rows, m.num_cols))


def abi_counts(m):
    """The definition at the C ABI, for a square matrix whose rows are sets N(v) -> (total, per as uint64[n]):
      total  = sum over v, over u in N(v), of |N(v) & N(u)|            = ((L L^T) o L).sum()
      per[x] = triples (v, u, w), u in N(v), w in N(v) & N(u), in which x is v, u or w: three sparse products --
               C = (L L^T) o L holds the w's of every pair (v, u): its row sums credit v, its column sums u;
               (L L) o L holds the u's of every pair (v, w): its column sums credit w."""
    L = _pattern(m)
    assert L.shape[0] == L.shape[1] and (L.nnz == 0 or L.data.max() == 1)
    C = (L @ L.T).multiply(L)
    W = (L @ L).multiply(L)
    per = np.asarray(C.sum(axis=1)).ravel() + np.asarray(C.sum(axis=0)).ravel() + np.asarray(W.sum(axis=0)).ravel()
    return int(C.sum()), per.astype(np.uint64)


def symmetric_simple(m):
    """the undirected simple graph of a matrix as a symmetric scipy pattern of int64 ones over n = max(rows, cols) vertices: an
    edge {u, v} iff u != v and a stored non-zero entry A[v, u] or A[u, v] exists"""
    import scipy.sparse as sp
    n, nnz = max(m.num_rows, m.num_cols), m.nnz
    A = sp.csr_matrix((m.adj_data[:nnz] != 0, m.adj_indices[:nnz].astype(np.int64), m.adj_indptr.astype(np.int64)),
                      shape=(m.num_rows, m.num_cols))
    A.resize((n, n))
    A.eliminate_zeros()
    S = (A + A.T).tocsr()
    S.setdiag(False)
    S.eliminate_zeros()
    return sp.csr_matrix((np.ones(S.nnz, np.int64), S.indices, S.indptr), shape=(n, n))


def triangles_by_definition(m):
    """The definition at the drivers -> (triangles through every vertex as uint64[n], undirected degrees as int64[n]):
    ((S S) o S) row sums / 2 on the symmetric pattern S: a closed walk v-u-w-v is counted for (u, w) and (w, u)."""
    S = symmetric_simple(m)
    twice = np.asarray((S @ S).multiply(S).sum(axis=1)).ravel()
    assert not np.any(twice & 1)
    return (twice // 2).astype(np.uint64), np.asarray(S.sum(axis=1)).ravel().astype(np.int64)


def _nx_graph(m):
    import networkx as nx
    S = symmetric_simple(m).tocoo()
    G = nx.Graph()
    G.add_nodes_from(range(S.shape[0]))
    G.add_edges_from(zip(S.row.tolist(), S.col.tolist()))
    return G


def _csr(n, rows, cols, data=None):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    data = np.ones(rows.shape[0], np.float32) if data is None else np.asarray(data, np.float32)[order]
    return io.CSRMatrix(n, n, data, cols.astype(np.uint32), np.cumsum(indptr).astype(np.uint32))


def messy_graph(seed=3):
    """2000 vertices: random entries with duplicates, a diagonal, zero-valued entries (some the only copy of their edge) and one-way
    storage -- everything the drivers ignore -- padded to 2048"""
    rng = np.random.default_rng(seed)
    n, e = 2000, 30000
    rows, cols = rng.integers(0, n, e), rng.integers(0, n, e)
    rows, cols = np.concatenate([rows, rows[:3000], np.arange(0, n, 7)]), np.concatenate([cols, cols[:3000], np.arange(0, n, 7)])
    data = np.where(rng.random(rows.shape[0]) < 0.15, 0.0, rng.random(rows.shape[0]) + 0.5)
    return _csr(2048, rows, cols, data)


def test_library_exports_and_binds_the_entry_point():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "graphlily_hip.h")).read()
    assert hasattr(L, "gl_tc_count"), "libgraphlily_hip.so does not export gl_tc_count"
    assert "gl_tc_count" in capi.EXPORTS and len(L.gl_tc_count.argtypes) == 3
    assert DECL in header
    assert callable(capi.SpMVPlan.tc_count) and callable(M.SpMVModule.tc_count) and callable(io.triangle_orient)
    assert callable(app.TriangleCount.run) and callable(app.TriangleCount.clustering) and callable(app.validate_triangles)
    assert "tc_count(DeviceBuffer total, uint64_t *per_vertex = nullptr)" in open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    tc_h = open(os.path.join(ROOT, "include", "graphlily", "app", "tc.h")).read()
    for piece in ("class TriangleCount", "run()", "num_triangles()", "transitivity()", "util_triangle_orient"):
        assert piece in tc_h
    assert "util_triangle_orient" in open(os.path.join(ROOT, "include", "graphlily", "io", "data_formatter.h")).read()


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_tc_count(None, None, None) == capi.GL_ERR_NOT_INITIALIZED


GRAPHS = {
    "uniform": lambda: datasets.uniform(3000, 6, seed=5),
    "rmat": lambda: datasets.rmat(4000, 30000, seed=6),
    "rmat_sym": lambda: datasets.rmat(4000, 40000, seed=8, symmetric=True),
    "messy": messy_graph,
    "many": lambda: many_components(),
}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_definition_agrees_with_networkx(graph):
    import networkx as nx
    m = GRAPHS[graph]()
    if graph == "many":                       # 90 000 vertices: too many for networkx; only the cycles of three vertices are triangles
        t, deg = triangles_by_definition(m)
        assert int(t.sum()) == 3 * MANY_CYCLES[3] > 0 and t.max() == 1 and deg.max() == 199
        total, per = abi_counts(io.triangle_orient(m)[0])
        assert total == MANY_CYCLES[3] and np.array_equal(per, t)
        return
    assert max(m.num_rows, m.num_cols) <= 4096
    t, deg = triangles_by_definition(m)
    G = _nx_graph(m)
    want = nx.triangles(G)
    assert np.array_equal(t, np.array([want[v] for v in range(t.shape[0])], dtype=np.uint64))
    assert np.array_equal(deg, np.array([G.degree(v) for v in range(t.shape[0])]))
    assert t.sum() % 3 == 0 and t.sum() > 0
    # the oriented matrix at the ABI gives the same counts, every triangle once, and the symmetric one six times
    o, odeg = io.triangle_orient(m)
    total, per = abi_counts(o)
    assert total == int(t.sum()) // 3 and np.array_equal(per, t) and np.array_equal(odeg, deg)
    sym = _from_scipy(symmetric_simple(m))
    stotal, sper = abi_counts(sym)
    assert stotal == 6 * total and np.array_equal(sper, 6 * t)
    # transitivity and clustering as the driver computes them (CPU stand-in for the device: the driver's host arithmetic only)
    wedges = int((deg * (deg - 1) // 2).sum())
    assert 3.0 * total / wedges == pytest.approx(nx.transitivity(G), rel=1e-12)
    tc = app.TriangleCount(backend=CpuBackend())
    tc.load_and_format_matrix(m)
    tc.triangles_ = np.concatenate([t, np.zeros(tc.n_ - t.shape[0], np.uint64)])
    c = tc.clustering()
    cw = nx.clustering(G)
    assert c.dtype == np.float64 and c.shape == (tc.n_,)
    np.testing.assert_allclose(c[:t.shape[0]], np.array([cw[v] for v in range(t.shape[0])]), rtol=1e-12, atol=0)
    assert not c[:t.shape[0]][deg < 2].any() and not c[t.shape[0]:].any()


# many_components(): how many of its 300 cycles have two vertices (one doubled edge) and three (a triangle)
_sizes = np.random.default_rng(31).integers(2, 201, size=900)[300:600]
MANY_CYCLES = {2: int(np.count_nonzero(_sizes == 2)), 3: int(np.count_nonzero(_sizes == 3))}


def _from_scipy(S):
    S = S.tocsr()
    S.sort_indices()
    return io.CSRMatrix(S.shape[0], S.shape[1], np.ones(S.nnz, np.float32), S.indices.astype(np.uint32), S.indptr.astype(np.uint32))


def test_abi_formula_with_a_diagonal_and_on_cliques():
    # K_5 as an upper triangle: C(5,3) triangles once, C(4,2) through every vertex; in full: six times
    iu = np.triu_indices(5, 1)
    up = _csr(8, iu[0], iu[1])
    total, per = abi_counts(up)
    assert total == 10 and np.array_equal(per, np.array([6] * 5 + [0] * 3, dtype=np.uint64))
    full = _csr(8, np.concatenate(iu), np.concatenate(iu[::-1]))
    assert abi_counts(full)[0] == 60
    o, deg = io.triangle_orient(full)          # (all degrees are equal: the orientation is by vertex number, the upper triangle)
    assert np.array_equal(o.adj_indices, up.adj_indices) and np.array_equal(o.adj_indptr, up.adj_indptr) and np.array_equal(deg[:5], [4] * 5)
    # a diagonal entry simply takes part: N(0) = {0, 1}, N(1) = {1}: the triples (0,0,0), (0,0,1), (0,1,1), (1,1,1)
    d = _csr(4, [0, 0, 1], [0, 1, 1])
    total, per = abi_counts(d)
    assert total == 4 and np.array_equal(per, np.array([6, 6, 0, 0], dtype=np.uint64))


@pytest.mark.parametrize("graph", ["rmat_20K", "messy", "many", "uniform"])
def test_triangle_orient(graph):
    m = named_matrix(graph) if graph == "rmat_20K" else GRAPHS[graph]()
    if graph == "rmat_20K":
        io.util_round_csr_matrix_dim(m, 128, 128)
    before = (m.adj_indptr.copy(), m.adj_indices.copy(), m.adj_data.copy())
    o, deg = io.triangle_orient(m)
    assert all(np.array_equal(a, b) for a, b in zip(before, (m.adj_indptr, m.adj_indices, m.adj_data))), "the input is left alone"
    n = max(m.num_rows, m.num_cols)
    assert (o.num_rows, o.num_cols) == (n, n) and deg.dtype == np.uint32 and deg.shape == (n,)
    assert o.adj_data.dtype == np.float32 and np.all(o.adj_data == 1) and o.adj_indices.dtype == np.uint32
    S = symmetric_simple(m)
    assert np.array_equal(deg, np.asarray(S.sum(axis=1)).ravel())
    ip = o.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(ip))
    cols = o.adj_indices.astype(np.int64)
    inside = np.ones(cols.shape[0], bool)
    inside[ip[:-1][np.diff(ip) > 0]] = False                     # (the first entry of every non-empty row)
    assert np.all(cols[1:][inside[1:]] > cols[:-1][inside[1:]]), "rows are strictly ascending"
    d = deg.astype(np.int64)
    assert np.all((d[cols] > d[rows]) | ((d[cols] == d[rows]) & (cols > rows))), "(deg[u], u) > (deg[v], v)"
    O = _pattern(o)
    assert ((O + O.T) != S).nnz == 0 and o.nnz * 2 == S.nnz, "every undirected edge is kept, in exactly one direction"
    total = abi_counts(o)[0]
    assert abi_counts(_from_scipy(S))[0] == 6 * total
    if graph == "rmat_20K":
        assert total == 6312502
        longest = int(np.diff(ip).max())
        assert longest == 165 and int(d.max()) == 5133 and longest * 20 < int(d.max())
    if graph == "many":
        A = _pattern(m)
        assert (A != A.T).nnz > 0, "entries are stored one way only"
        assert total == MANY_CYCLES[3] and o.nnz == m.nnz - MANY_CYCLES[2]      # (a cycle of two vertices stores its one edge twice)
    if graph == "messy":
        assert np.any(m.adj_data == 0) and np.any(np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64))) == m.adj_indices)
        assert o.nnz * 2 < m.nnz * 2 and total > 0
        assert not deg[2000:].any() and not np.diff(ip)[2000:].any(), "padding vertices have empty rows"


def test_validate_triangles():
    m = GRAPHS["messy"]()
    t, _ = triangles_by_definition(m)
    assert app.validate_triangles(m, t) == int(t.sum()) // 3
    assert app.validate_triangles(m, np.concatenate([t, np.zeros(64, np.uint64)])) == int(t.sum()) // 3     # (a padded array)
    k = int(np.flatnonzero(t)[5])
    for delta in (1, -1):
        bad = t.astype(np.int64)
        bad[k] += delta
        with pytest.raises(ValueError, match=r"vertex %d is given %d triangles, it lies in %d" % (k, int(t[k]) + delta, int(t[k]))):
            app.validate_triangles(m, bad)
    with pytest.raises(ValueError, match="counts for a"):
        app.validate_triangles(m, t[:100])


class _TwoRanks:
    """what the drivers ask of a communicator, claiming rank 0 of 2"""
    rank, world_size, distributed = 0, 2, True


def test_driver_refuses_row_shards_and_a_run_before_send(golden_dir):
    with pytest.raises(NotImplementedError, match="row shards"):
        app.TriangleCount(comm=_TwoRanks(), backend=CpuBackend())
    tc = app.TriangleCount(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        tc.run()
    tc.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (tc.n_, tc.n_real_) == (128, 8) and tc.degrees_.shape == (128,) and tc.degrees_[:8].max() == 2 and not tc.degrees_[8:].any()
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        tc.run(per_vertex=False)
    with pytest.raises(RuntimeError, match="per_vertex=True"):
        tc.clustering()


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("tc_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([TC_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
