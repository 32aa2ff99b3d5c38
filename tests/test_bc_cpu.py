"""CPU suite of the betweenness centrality (gl_bc_accumulate, SpMVPlan.bc_accumulate, SpMVModule.bc_accumulate, io.simple_pattern,
app.BetweennessCentrality, app.betweenness_by_levels, app.validate_betweenness): the export and its bindings exist, the preparation
gives simple sorted patterns and the right transpose, the host restatement of the definition meets networkx and the closed forms,
the validator accepts networkx's values and refuses three kinds of miss, the driver refuses what it cannot do, and the C++ driver
compiles against include/ and prepares the pattern like the Python function.  tests/test_gpu_bc.py compares the kernels with the
host restatement kept in app.betweenness_by_levels.

THE TOLERANCE is derived, not measured: every term of every sum is >= 0, so nothing cancels, and a value's relative error is at
most the number of roundings on its longest dependency chain times 2^-53: bound = 4 (D (longest row + 4) + sources) 2^-53 from the
case's own depth D, longest row and source count; the 4 covers two computations that round independently."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver, named_matrix
from test_kcore_cpu import _TwoRanks, _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC_DRIVER = os.path.join(ROOT, "build", "bc_driver")
DECL = ("int gl_bc_accumulate(gl_spmv_plan plan_in, gl_spmv_plan plan_out, const float *d_level, double *d_bc, double scale, int accumulate,\n"
        "                     double *d_sigma /* may be NULL: plan scratch */,\n"
        "                     uint32_t *h_stats /* may be NULL; 4 HOST words: depth D, reached vertices, orphans, non-finite sigmas */);")


def bound_of(depth, longest_row, num_sources):
    return 4.0 * (depth * (longest_row + 4) + num_sources) * 2.0 ** -53


def assert_close(got, want, bound, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.all(np.isfinite(got)), what
    assert np.array_equal(got == 0, want == 0), "%s: the zero patterns differ, first at %d" % (what, int(np.flatnonzero((got == 0) != (want == 0))[0]))
    miss = ~(np.abs(got - want) <= bound * want)
    assert not miss.any(), "%s: vertex %d: got %r, want %r (bound %.3g)" % (what, int(np.flatnonzero(miss)[0]), got[miss][0], want[miss][0], bound)


def digraph(n, src, dst, undirected=False):
    """edges src[i] -> dst[i] on n vertices as the matrix the drivers read: an entry A[v, u] is the edge u -> v"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    if undirected:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    return _csr(n, dst, src)


def longest_row(cin, cout):
    rows = [np.diff(m.adj_indptr.astype(np.int64)) for m in (cin, cout) if m is not None]
    return max(int(r.max()) if r.size else 0 for r in rows)


def host_bc(cin, cout, sources, n, scale=1.0):
    """-> (bc, per-source depths, per-source reached counts): the host restatement summed over single-source searches"""
    A_out = app._pattern_as_scipy(cin if cout is None else cout, n)
    bc, depths, reached = np.zeros(n, np.float64), [], []
    for s in sources:
        level = app._bfs_levels_of(A_out, [s], n)
        _, delta = app.betweenness_by_levels(cin, cout, level)
        bc += np.where(level >= 2, scale * delta, 0.0)
        depths.append(int(level.max()))
        reached.append(int(np.count_nonzero(level)))
    return bc, depths, reached


def nx_bc(cin, cout, n, normalized, nodes=None):
    """networkx.betweenness_centrality of the pattern (cout None: undirected) -> float64[n]; `nodes`: of the subgraph they induce
    (whole components: the values of their vertices are those in the whole graph)"""
    import networkx as nx
    G = nx.Graph() if cout is None else nx.DiGraph()
    G.add_nodes_from(range(n) if nodes is None else nodes)
    rows = np.repeat(np.arange(cin.num_rows), np.diff(cin.adj_indptr.astype(np.int64)))
    keep = np.ones(rows.shape[0], bool) if nodes is None else np.isin(rows, np.asarray(list(nodes)))
    G.add_edges_from(zip(cin.adj_indices[keep].tolist(), rows[keep].tolist()))       # u -> v for an entry A[v, u]
    got = nx.betweenness_centrality(G, normalized=normalized)
    out = np.zeros(n, np.float64)
    for v, x in got.items():
        out[v] = x
    return out


@functools.lru_cache(maxsize=None)
def prepared(name):
    """-> (the matrix as given, padded to 128, csr_in, csr_out or None, directed); computed once and shared, never written"""
    from test_cc_cpu import many_components
    if name in ("line_8", "eye_10"):
        raw = io.load_csr_matrix_from_float_npz(os.path.join(ROOT, "tests", "golden", name + "_csr_float32.npz"))
    elif name == "many":
        raw = many_components()
    else:
        raw = named_matrix(name)
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    cin, cout, directed = app._bc_patterns(m, None)
    return raw, m, cin, cout, directed


@functools.lru_cache(maxsize=None)
def many_sample():
    """`many` is a disjoint union of 900 small components on 91 392 vertices: all its sources are 90 789 searches -- a minute and
    a half on the host for the restatement and as long for networkx (measured), minutes of launches on the device.  A component's
    values do not depend on the other components, so the tests take ALL the sources of a sample of WHOLE components -- the
    shortest (>= 3 vertices) and the longest of at most 64 vertices among the paths, the cycles and the stars, and a two-vertex
    component -- and compare those components' vertices: every value there is the all-sources value of the whole graph.  -> (sources, one array of vertices per component)"""
    from scipy.sparse.csgraph import connected_components
    raw, m, cin, cout, directed = prepared("many")
    sym = io.symmetrize_simple(m)[0]
    n = sym.num_rows
    _, lab = connected_components(app._pattern_as_scipy(sym, n), directed=False)
    deg = np.diff(sym.adj_indptr.astype(np.int64))
    comps = {}
    for c in np.unique(lab[deg > 0]):
        v = np.flatnonzero(lab == c)
        d = deg[v]
        kind = "two" if v.size == 2 else "star" if d.max() > 2 else "cycle" if d.min() == 2 else "path"
        comps.setdefault(kind, []).append(v)
    picked = [comps["two"][0]]
    for kind in ("path", "cycle", "star"):
        by_size = sorted((c for c in comps[kind] if 3 <= c.size <= 64), key=lambda c: (c.size, int(c[0])))
        picked += [by_size[0], by_size[-1]]
    return [int(v) for c in picked for v in c], picked


# ---- closed forms (all sources, unnormalised; undirected ones carry networkx's 1/2) --------------------------------------------
def path_graph(k, n=None, first=0):
    v = np.arange(first, first + k)
    want = np.zeros(n or k)
    want[v] = np.arange(k) * (k - 1.0 - np.arange(k))
    return digraph(n or k, v[:-1], v[1:], True), want


def star_graph(leaves, n=None, centre=0):
    n = n or leaves + 1
    lv = np.array([v for v in range(leaves + 1) if v != centre]) if centre <= leaves else np.arange(leaves)
    want = np.zeros(n)
    want[centre] = leaves * (leaves - 1) / 2.0
    return digraph(n, np.full(leaves, centre), lv, True), want


def cycle_graph(k, n=None):
    v = np.arange(k)
    want = np.zeros(n or k)
    want[:k] = (k - 2.0) ** 2 / 8.0 if k % 2 == 0 else (k - 1.0) * (k - 3.0) / 8.0
    return digraph(n or k, v, np.roll(v, -1), True), want


def bipartite_graph(a, b, n=None):
    x, y = np.repeat(np.arange(a), b), np.tile(np.arange(a, a + b), a)
    want = np.zeros(n or a + b)
    want[:a] = b * (b - 1) / 2.0 / a
    want[a:a + b] = a * (a - 1) / 2.0 / b
    return digraph(n or a + b, x, y, True), want


def diamond_chain(k, n=None):
    """joint i = vertex 3 i, i = 0 .. k; diamond i: joint i -> 3 i + 1, 3 i + 2 -> joint i + 1 (directed).  -> (matrix, the
    all-sources betweenness, the dependency of source 0 alone)"""
    i = np.arange(k)
    src = np.concatenate([3 * i, 3 * i, 3 * i + 1, 3 * i + 2])
    dst = np.concatenate([3 * i + 1, 3 * i + 2, 3 * i + 3, 3 * i + 3])
    n = n or 3 * k + 1
    want, from0 = np.zeros(n), np.zeros(n)
    j = np.arange(k + 1)
    want[3 * j] = 9.0 * j * (k - j)
    mid = (3.0 * i + 1) * (3.0 * (k - i - 1) + 1) / 2.0
    want[3 * i + 1] = want[3 * i + 2] = mid
    from0[3 * j[1:]] = 3.0 * (k - j[1:])                 # every later vertex is reached through the joint
    from0[3 * i + 1] = from0[3 * i + 2] = (3.0 * (k - i - 1) + 1) / 2.0      # half the paths to joint i + 1 and beyond
    return digraph(n, src, dst), want, from0


def test_library_exports_and_binds_the_entry_point():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "graphlily_hip.h")).read()
    assert hasattr(L, "gl_bc_accumulate"), "libgraphlily_hip.so does not export gl_bc_accumulate"
    assert "gl_bc_accumulate" in capi.EXPORTS and len(capi.EXPORTS) == 113 and len(L.gl_bc_accumulate.argtypes) == 8
    assert DECL in header
    assert callable(capi.SpMVPlan.bc_accumulate) and callable(M.SpMVModule.bc_accumulate) and callable(io.simple_pattern)
    assert callable(app.BetweennessCentrality.run) and callable(app.betweenness_by_levels) and callable(app.validate_betweenness)
    assert "bc_accumulate(" in open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    bc_h = open(os.path.join(ROOT, "include", "graphlily", "app", "bc.h")).read()
    for piece in ("class BetweennessCentrality", "run(", "depths()", "reached()", "overflowed()", "util_simple_pattern"):
        assert piece in bc_h
    assert "util_simple_pattern" in open(os.path.join(ROOT, "include", "graphlily", "io", "data_formatter.h")).read()
    assert "gl_bc.hip" in open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    if capi.device_count() == 0:
        assert L.gl_bc_accumulate(None, None, None, None, 1.0, 0, None, None) == capi.GL_ERR_NOT_INITIALIZED


def _hand_made():
    """6 x 9: a duplicate, a diagonal entry, zero-valued entries, one-way and two-way entries, unsorted columns, a column beyond
    the rows"""
    rows = [0, 0, 0, 0, 1, 2, 2, 3, 3, 5, 5]
    cols = [3, 1, 1, 0, 4, 0, 5, 2, 0, 8, 2]
    data = [1, 2, 1, 7, 0, 0, 3, 1, 1, 1, 0]
    return _csr(6, rows, cols, data, num_cols=9)


def _rows_of(m):
    ip = m.adj_indptr.astype(np.int64)
    return {v: m.adj_indices[ip[v]:ip[v + 1]].tolist() for v in range(m.num_rows) if ip[v + 1] > ip[v]}


def test_simple_pattern_on_hand_made_matrices():
    m = _hand_made()
    before = (m.adj_indptr.copy(), m.adj_indices.copy(), m.adj_data.copy())
    cin, cout, sym = io.simple_pattern(m)
    assert all(np.array_equal(a, b) for a, b in zip(before, (m.adj_indptr, m.adj_indices, m.adj_data))), "the input is left alone"
    assert not sym and (cin.num_rows, cin.num_cols, cout.num_rows, cout.num_cols) == (9, 9, 9, 9)
    assert _rows_of(cin) == {0: [1, 3], 2: [5], 3: [0, 2], 5: [8]}          # duplicates, the diagonal and zero values are gone
    assert _rows_of(cout) == {0: [3], 1: [0], 2: [3], 3: [0], 5: [2], 8: [5]}
    for x in (cin, cout):
        assert x.adj_indptr.dtype == np.uint32 and x.adj_indices.dtype == np.uint32 and x.adj_data.dtype == np.float32
        assert np.all(x.adj_data == 1) and x.nnz == 6
    s = io.symmetrize_simple(m)[0]
    sin, sout, ssym = io.simple_pattern(s)
    assert ssym and sout is None and np.array_equal(sin.adj_indices, s.adj_indices) and np.array_equal(sin.adj_indptr, s.adj_indptr)
    e, eo, es = io.simple_pattern(_csr(4, [0, 1, 2], [0, 1, 2], [1, 0, 5]))      # only a diagonal: an empty graph is symmetric
    assert e.nnz == 0 and eo is None and es and np.array_equal(e.adj_indptr, np.zeros(5, np.uint32))


@pytest.mark.parametrize("graph,symmetric", [("rmat_20K", False), ("rmat_sym_50K", True)])
def test_simple_pattern_is_simple_sorted_and_transposed(graph, symmetric):
    import scipy.sparse as sp
    raw, m, cin, cout, directed = prepared(graph)
    assert io.simple_pattern(m)[2] == symmetric and directed == (not symmetric) and (cout is None) == symmetric
    n = max(m.num_rows, m.num_cols)
    A = sp.csr_matrix((m.adj_data[:m.nnz] != 0, m.adj_indices[:m.nnz].astype(np.int64), m.adj_indptr.astype(np.int64)), shape=(m.num_rows, m.num_cols))
    A.resize((n, n))
    A.setdiag(False)
    A.eliminate_zeros()
    for x, W in ((cin, A), (cout, A.T.tocsr())):
        if x is None:
            assert ((A != 0) != (A.T != 0)).nnz == 0
            continue
        ip = x.adj_indptr.astype(np.int64)
        rows, cols = np.repeat(np.arange(n), np.diff(ip)), x.adj_indices.astype(np.int64)
        inside = np.ones(cols.shape[0], bool)
        inside[ip[:-1][np.diff(ip) > 0]] = False                     # (the first entry of every non-empty row)
        assert np.all(cols[1:][inside[1:]] > cols[:-1][inside[1:]]), "rows are strictly ascending"
        assert not np.any(rows == cols)
        S = sp.csr_matrix((np.ones(x.nnz, bool), cols, ip), shape=(n, n))
        assert ((W != 0) != (S != 0)).nnz == 0, "exactly the edges of the matrix"


def _random_graph(directed, seed, n=400, e=2400):
    rng = np.random.default_rng(seed)
    return digraph(n, rng.integers(0, n, e), rng.integers(0, n, e), not directed)


@pytest.mark.parametrize("case", ["directed_400", "undirected_400", "line_8"])
def test_host_restatement_equals_networkx(case):
    if case == "line_8":
        m = prepared("line_8")[1]
    else:
        m = _random_graph(case == "directed_400", 3)
    cin, cout, directed = app._bc_patterns(m, None)
    assert directed == (case != "undirected_400")                    # (line_8 stores every edge one way)
    n = cin.num_rows
    got, depths, _ = host_bc(cin, cout, range(n), n, 1.0 if directed else 0.5)
    assert_close(got, nx_bc(cin, cout, n, False), bound_of(max(depths), longest_row(cin, cout), n), case)
    assert got.max() > 0


def test_host_restatement_equals_networkx_on_whole_components_of_many():
    raw, m, cin, cout, directed = prepared("many")
    assert directed and cout is not None                             # every edge is stored one way only
    sym = io.symmetrize_simple(m)[0]
    n = sym.num_rows
    sources, comps = many_sample()
    A = app._pattern_as_scipy(sym, n)
    got, depth = np.zeros(n), 1
    # one source from every sampled component per round: the components are disjoint, so every component sees ONE source
    for r in range(max(c.size for c in comps)):
        level = app._bfs_levels_of(A, [int(c[r]) for c in comps if c.size > r], n)
        _, delta = app.betweenness_by_levels(sym, None, level)
        got += np.where(level >= 2, 0.5 * delta, 0.0)
        depth = max(depth, int(level.max()))
    bound = bound_of(depth, longest_row(sym, None), max(c.size for c in comps))
    for c in comps:
        assert_close(got[c], nx_bc(sym, None, n, False, nodes=c.tolist())[c], bound, "component of %d" % c.size)
    k = comps[-1].size - 1                                           # the largest star's centre: C(leaves, 2)
    assert abs(got[comps[-1]].max() - k * (k - 1) / 2.0) <= bound * k * (k - 1) / 2.0


@pytest.mark.parametrize("case", ["P_9", "P_40", "star_50", "C_8", "C_9", "K_7_30", "diamonds_5"])
def test_host_restatement_meets_the_closed_forms(case):
    kind, *k = case.split("_")
    k = [int(x) for x in k]
    from0 = None
    if kind == "P":
        m, want = path_graph(k[0])
    elif kind == "star":
        m, want = star_graph(k[0])
    elif kind == "C":
        m, want = cycle_graph(k[0])
    elif kind == "K":
        m, want = bipartite_graph(k[0], k[1])
    else:
        m, want, from0 = diamond_chain(k[0])
    cin, cout, directed = app._bc_patterns(m, None)
    assert directed == (kind == "diamonds")
    n = cin.num_rows
    got, depths, _ = host_bc(cin, cout, range(n), n, 1.0 if directed else 0.5)
    bound = bound_of(max(depths), longest_row(cin, cout), n)
    assert_close(got, want, bound, case)
    assert_close(got, nx_bc(cin, cout, n, False), bound, case + " (networkx)")
    if from0 is not None:                                            # the single-source form tests/test_gpu_bc.py uses
        one, d, _ = host_bc(cin, cout, [0], n)
        assert_close(one, from0, bound, case + " from 0")
        level = app._bfs_levels_of(app._pattern_as_scipy(cout, n), [0], n)
        sigma, _ = app.betweenness_by_levels(cin, cout, level)
        assert np.array_equal(sigma[::3], 2.0 ** np.arange(k[0] + 1)) and d == [2 * k[0] + 1]


@pytest.mark.parametrize("directed", [True, False])
@pytest.mark.parametrize("normalized", [True, False])
def test_validate_betweenness_accepts_networkx_and_refuses_misses(directed, normalized):
    m = _random_graph(directed, 5, 120, 500)                         # (every validation is 120 searches on the host)
    cin, cout, d = app._bc_patterns(m, None)
    n = cin.num_rows
    want = nx_bc(cin, cout, n, normalized)
    err = app.validate_betweenness(m, want, normalized=normalized)
    assert 0 <= err < 1e-9                                           # (the validator derives its bound from its own searches)
    padded = np.concatenate([want, np.zeros(112)])                   # (an array longer than the matrix: the drivers pad)
    assert app.validate_betweenness(m, padded, normalized=normalized, directed=d) == err
    bad = want.copy()
    v = int(np.argmax(want))
    bad[v] *= 1.0 + 1e-9
    with pytest.raises(ValueError, match="vertex %d is given" % v):
        app.validate_betweenness(m, bad, normalized=normalized)
    with pytest.raises(ValueError, match="is given"):
        app.validate_betweenness(m, want * 2.0, normalized=normalized)           # a wrong scale
    with pytest.raises(ValueError, match="is given"):
        app.validate_betweenness(m, want, normalized=not normalized)
    padded[n + 5] = 1e-300
    with pytest.raises(ValueError, match="padding vertex %d" % (n + 5)):
        app.validate_betweenness(m, padded, normalized=normalized)
    zero = want.copy()
    zero[v] = 0.0
    with pytest.raises(ValueError, match="vertex %d is given 0, its" % v):
        app.validate_betweenness(m, zero, normalized=normalized)
    with pytest.raises(ValueError, match="values for a"):
        app.validate_betweenness(m, want[:100], normalized=normalized)
    if directed:            # read as undirected: every edge in both directions
        und = nx_bc(io.symmetrize_simple(m)[0], None, n, normalized)
        assert app.validate_betweenness(m, und, normalized=normalized, directed=False) < 1e-9


def test_scale_is_networkx_rescale():
    from networkx.algorithms.centrality.betweenness import _rescale
    for n in (1, 2, 3, 10):
        for k in (1, 2, n):
            if k > n:
                continue
            for normalized in (True, False):
                for directed in (True, False):
                    want = _rescale({0: 1.0}, n, normalized, directed=directed, k=None if k == n else k)[0]
                    assert app._bc_scale(n, k, normalized, directed) == want, (n, k, normalized, directed)


def test_driver_refuses_row_shards_and_a_run_before_send(golden_dir):
    with pytest.raises(NotImplementedError, match="row shards"):
        app.BetweennessCentrality(comm=_TwoRanks(), backend=CpuBackend())
    bc = app.BetweennessCentrality(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        bc.run()
    bc.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (bc.n_, bc.n_real_) == (128, 8) and bc.directed_ in (True, False)
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        bc.run(sources=[0])
    und = app.BetweennessCentrality(backend=CpuBackend())
    und.load_and_format_matrix(prepared("rmat_20K")[0], directed=False)
    assert und.directed_ is False and und.out_ is None
    two = app.BetweennessCentrality(backend=CpuBackend())
    two.load_and_format_matrix(prepared("uniform_10K_10")[0], directed=True)
    assert two.directed_ is True and two.out_ is not None


def save_npz(m, path):
    import scipy.sparse as sp
    A = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int32), m.adj_indptr.astype(np.int32)), shape=(m.num_rows, m.num_cols), dtype=np.float32)
    sp.save_npz(path, A, compressed=False)


def test_cpp_driver_compiles_and_prepares_the_pattern_alike(tmp_path):
    build_cpp_driver("bc_driver.cpp")
    raw = prepared("rmat_20K")[0]
    path = str(tmp_path / "rmat_20K_csr_float32.npz")
    save_npz(raw, path)
    r = subprocess.run([BC_DRIVER, "--pattern", path, str(tmp_path)], capture_output=True, text=True, timeout=120)     # host only
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _, m, cin, cout, _ = prepared("rmat_20K")
    assert "symmetric: 0" in r.stdout and "shape: %d %d" % (cin.num_rows, cin.num_cols) in r.stdout
    for name, want in (("in", cin), ("out", cout)):
        assert np.array_equal(np.fromfile(str(tmp_path / ("cpp_%s_indptr.bin" % name)), dtype=np.uint32), want.adj_indptr)
        assert np.array_equal(np.fromfile(str(tmp_path / ("cpp_%s_indices.bin" % name)), dtype=np.uint32), want.adj_indices)
    if capi.device_count() == 0:
        r = subprocess.run([BC_DRIVER, str(tmp_path / "none.npz"), str(tmp_path), "0"], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
