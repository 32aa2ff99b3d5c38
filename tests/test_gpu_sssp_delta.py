"""GPU parity of delta-stepping shortest paths (gl_sssp_delta, SpMVPlan.sssp_delta, app.ShortestPaths, graphlily::app::ShortestPaths)
against a plain Dijkstra in f32 on the host (dijkstra_f32 below).  dist is the unique least fixed point of f32 relaxation, parent
and the orphan count follow from it, so every comparison is exact, dist as 32-bit words -- under every delta, which only changes the
schedule.  On the integer-weight cases the host reference is itself checked once against scipy's f64 Dijkstra (sums below 2^24 are
exact in f32).  The wording of this kernel's refusals is tested here (test_refusals); tests/test_gpu_rows.py calls it before and
behind every other asker of the cached verdicts and of the transpose-partner cache, tests/test_gpu_rounds.py runs it before and
behind the other users of rounds_run and of the staging words (sssp_delta_batch 1 and default), and
tests/test_gpu_walk.py::test_sssp_delta runs its two walk sites on the star union at the cuts 0, 4, 8 and the default."""
import functools
import heapq
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph

from graphlily_amd import app, capi, datasets, io, module as M

from helpers import build_cpp_driver, set_knob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, INF_BITS, GARBAGE = 0xFFFFFFFF, 0x7F800000, 0xDEADBEEF
DELTAS = ("tiny", "default", "one", "huge", "inf")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def dijkstra_f32(g_in, sources):
    """-> (dist float32[n], parent uint32[n], orphans) on the graph whose row v lists the predecessors u of v with w(u -> v)"""
    n = g_in.num_rows
    rows = np.repeat(np.arange(n), np.diff(g_in.adj_indptr.astype(np.int64)))
    cols, w = g_in.adj_indices.astype(np.int64), g_in.adj_data.astype(np.float32)
    succ = [[] for _ in range(n)]
    for v, u, x in zip(rows.tolist(), cols.tolist(), w):
        succ[u].append((v, x))
    sources = np.asarray(sources, dtype=np.int64)
    dist = np.full(n, np.inf, dtype=np.float32)
    dist[sources] = 0
    heap = [(0.0, s) for s in sources.tolist()]
    with np.errstate(over="ignore"):                               # (a sum may overflow to inf: unreached)
        while heap:
            d, u = heapq.heappop(heap)
            for v, x in succ[u] if d == dist[u] else ():
                if np.float32(dist[u] + x) < dist[v]:
                    dist[v] = np.float32(dist[u] + x)
                    heapq.heappush(heap, (float(dist[v]), v))
        fits = np.isfinite(dist[rows]) & (dist[cols] < dist[rows]) & (dist[cols] + w == dist[rows])
    parent = np.full(n, NONE, dtype=np.int64)
    np.minimum.at(parent, rows[fits], cols[fits])
    parent[sources] = sources
    return dist, parent.astype(np.uint32), int(np.count_nonzero(np.isfinite(dist) & (parent == NONE)))


def _csr(n, v, u, w):
    """entries A[v, u] = w (an edge u -> v), in any order"""
    v, u = np.asarray(v, dtype=np.int64), np.asarray(u, dtype=np.int64)
    m = sp.coo_matrix((np.ones(len(v)), (v, u)), shape=(n, n)).tocsr()      # (the pattern: a stored 0 must stay stored)
    assert m.nnz == len(v), "the cases hold every edge once"
    order = np.lexsort((u, v))
    return io.CSRMatrix(n, n, np.asarray(w, dtype=np.float32)[order], m.indices.astype(np.uint32), m.indptr.astype(np.uint32))


def _weighted(m, seed, kinds=255):
    w = np.random.default_rng(seed).integers(1, kinds + 1, size=m.nnz).astype(np.float32)
    return io.CSRMatrix(m.num_rows, m.num_cols, w, m.adj_indices, m.adj_indptr)


def _grid(k, seed):
    at = np.arange(k * k).reshape(k, k)
    a = np.concatenate([at[:, :-1].ravel(), at[:-1, :].ravel()])
    b = np.concatenate([at[:, 1:].ravel(), at[1:, :].ravel()])
    v, u = np.concatenate([a, b]), np.concatenate([b, a])                   # symmetric pattern, a weight per direction
    return _csr(k * k, v, u, np.random.default_rng(seed).integers(1, 256, size=v.size))


def _case(name):
    """-> (matrix, sources, weighted)"""
    rng = np.random.default_rng(11)
    if name == "path_2000":                      # one way: plan_out != plan_in, many buckets, many batches, buckets jumped
        return _csr(2000, np.arange(1, 2000), np.arange(1999), rng.integers(1, 8, size=1999)), [0], True
    if name == "star":                           # hub 0 with 5000 leaves, vertex 1 with 300 more; the source is a leaf of the hub
        v = np.concatenate([np.arange(1, 5001), np.zeros(5000, int), np.arange(5001, 5301), np.ones(300, int)])
        u = np.concatenate([np.zeros(5000, int), np.arange(1, 5001), np.ones(300, int), np.arange(5001, 5301)])
        return _csr(5301, v, u, rng.integers(1, 6, size=v.size)), [4999], True
    if name == "grid_40":
        return _grid(40, 5), [820], True
    if name.startswith("rmat"):                  # rmat[_sym]_{w255,unit}[_3src]
        m = datasets.rmat(4096, 65536, 3, symmetric="_sym" in name)
        return (_weighted(m, 4) if "w255" in name else m), ([0, 77, 4000] if "3src" in name else [int(np.argmax(np.diff(m.adj_indptr)))]), "w255" in name
    if name == "zero_cycle":                     # 0 -3-> 1 -2-> 2, a cycle 2 -> 3 -> 4 -> 2 of zeros, 4 -1-> 5; 6, 7 apart
        return _csr(8, [1, 2, 3, 4, 2, 5, 7], [0, 1, 2, 3, 4, 4, 6], [3, 2, 0, 0, 0, 1, 1]), [0], True
    if name == "all_zero":
        m = datasets.rmat(512, 4096, 9, symmetric=False)
        return io.CSRMatrix(512, 512, np.zeros(m.nnz, np.float32), m.adj_indices, m.adj_indptr), [int(np.argmax(np.diff(m.adj_indptr)))], True
    if name == "huge_1e30":                      # with delta = 1 everything lies in the clamped top bucket, and heavy edges stay in it
        g = _grid(6, 8)
        return io.CSRMatrix(36, 36, g.adj_data * np.float32(1e30), g.adj_indices, g.adj_indptr), [0], True
    if name == "reopened":                       # a chain h_0 .. h_24 of 1e30 edges; h_i -> c_1 weighs 1e33 - 2e30 i, so with delta = 1
        k = m = 24                               # -- all in the clamped top bucket -- every epoch lowers c_1 once more and re-runs the
        h, c = np.arange(k + 1), k + 1 + np.arange(m)      # zero-weight chain c_1 .. c_24 behind it: about k (m + 1) = 600 steps for n_ = 128
        v = np.concatenate([h[1:], np.full(k + 1, c[0]), c[1:]])
        u = np.concatenate([h[:-1], h, c[:-1]])
        w = np.concatenate([np.full(k, 1e30), 1e33 - 2e30 * h, np.zeros(m - 1)])
        return _csr(k + 1 + m, v, u, w), [0], True
    if name == "absorbed":                       # 0 -1-> 1 -2^-149-> 2 -2^-149-> 1, 2 -1-> 3: the tiny weights lower nothing behind 1.0
        t = np.float32(2.0 ** -149)
        return _csr(4, [1, 2, 1, 3], [0, 1, 2, 2], [1, t, t, 1]), [0], True
    if name == "overflow":                       # 3e38 + 3e38 = inf: vertex 2 is unreached
        return _csr(3, [1, 2], [0, 1], [3e38, 3e38]), [0], True
    if name == "isolated_source":
        return _csr(70, [1, 2], [0, 1], [1, 1]), [69], True
    raise KeyError(name)


CASES = ["path_2000", "star", "grid_40", "rmat_w255", "rmat_unit", "rmat_sym_w255", "rmat_sym_unit_3src", "zero_cycle", "all_zero",
         "huge_1e30", "reopened", "absorbed", "overflow", "isolated_source"]
INTEGER = CASES[:7]


@functools.lru_cache(maxsize=None)
def _loaded(name):
    """-> (driver, sources, reference): one load and one host Dijkstra per case, shared by every test and never changed"""
    m, sources, weighted = _case(name)
    d = app.ShortestPaths(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True, weighted)
    d.send_matrix_host_to_device()
    return d, sources, dijkstra_f32(d.graph_, sources)


def _delta(kind, d, ref):
    w = d.graph_.adj_data
    if kind == "tiny":                           # below the smallest positive weight: every positive edge is heavy
        least = w[w > 0].min() if np.any(w > 0) else np.float32(2e-30)
        return least / 2 if least / 2 > 0 else least            # (half of 2^-149 is 0: the weight itself, which is still heavy)
    if kind == "huge":                           # above the longest path: one bucket, but a finite width
        return np.float32(min(2.0 * float(ref[0][np.isfinite(ref[0])].max()) + 1.0, 3e38))
    return {"default": None, "one": 1.0, "inf": np.inf}[kind]


def _check(d, sources, ref, delta):
    got = d.run(sources if len(sources) > 1 else sources[0], delta)
    want, parent, orphans = ref
    assert np.array_equal(bits(got), bits(want)), "dist: first difference at vertex %d" % int(np.flatnonzero(bits(got) != bits(want))[0])
    assert np.array_equal(d.parent_, parent), "parent: first difference at vertex %d" % int(np.flatnonzero(d.parent_ != parent)[0])
    assert d.orphans_ == orphans and d.reached_ == int(np.isfinite(want).sum()) and d.launches_ >= 1
    if delta is not None and np.isinf(delta):
        assert d.buckets_ == 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DELTAS)
@pytest.mark.parametrize("name", CASES)
def test_every_case_under_every_delta(gpu, name, kind):
    d, sources, ref = _loaded(name)
    _check(d, sources, ref, _delta(kind, d, ref))
    if name == "zero_cycle":
        assert d.orphans_ == 2 and list(d.path(5)) == [5, 4] and list(d.path(2)) == [2, 1, 0] and list(d.path(7)) == []      # 3 and 4: orphans
    if name == "overflow":
        assert bits(d.dist_)[2] == INF_BITS and d.reached_ == 2


@pytest.mark.parametrize("name", INTEGER)
def test_the_host_reference_equals_scipy_in_f64(name):
    m, sources, weighted = _case(name)
    g_in = io.directed_weighted(m, weighted, "smallest")[0]
    a = sp.csr_matrix((g_in.adj_data.astype(np.float64), g_in.adj_indices, g_in.adj_indptr), shape=(g_in.num_rows,) * 2)
    want = sp.csgraph.dijkstra(a.T.tocsr(), indices=sources, min_only=True)
    assert np.array_equal(dijkstra_f32(g_in, sources)[0].astype(np.float64), want) and np.isfinite(want).sum() > 1


@pytest.mark.gpu
def test_unit_weights_equal_bfs_levels(gpu):
    d, sources, ref = _loaded("rmat_unit")
    bfs = app.BFS(M.num_hbm_channels, 1024, 512, 256)
    bfs.set_target("hw")
    bfs.set_up_runtime("unused.xclbin")
    bfs.load_and_format_matrix(_case("rmat_unit")[0], True)
    bfs.send_matrix_host_to_device()
    level = bfs.pull_push(sources[0], 64, 0.05)
    assert np.array_equal(bits(np.where(level > 0, level - 1, np.inf)), bits(d.run(sources[0]))) and level.max() > 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_40", "rmat_w255"])
def test_bellman_ford_driver_agrees_on_the_reached_vertices(gpu, name):
    d, sources, ref = _loaded(name)
    s = app.SSSP(M.num_hbm_channels, 1024, 512, 256)
    s.set_target("hw")
    s.set_up_runtime("unused.xclbin")
    s.load_and_format_matrix(_case(name)[0], True, weighted=True)
    s.send_matrix_host_to_device()
    got = s.pull(sources[0], s.n_)
    got = np.where(got >= np.float32(M.FLOAT_INF), np.float32(np.inf), got)
    assert np.array_equal(bits(got), bits(d.run(sources[0])))


@pytest.mark.gpu
def test_knobs_change_nothing(gpu, monkeypatch):
    for key, value in (("sssp_delta_cut", 0), ("sssp_delta_grid", 1), ("sssp_delta_batch", 1)):
        set_knob(monkeypatch, key, value)
    for name in ("star", "rmat_w255"):
        d, sources, ref = _loaded(name)
        _check(d, sources, ref, None)


def _plans(m):
    g_in, g_out, symmetric = io.directed_weighted(m, True, "smallest")
    plan = lambda g: capi.SpMVPlan(g.num_rows, g.num_cols, g.adj_indptr, g.adj_indices, np.ones(g.nnz, np.float32), 0, g.num_rows, flags=capi.GL_PLAN_BOOLEAN)
    return g_in, g_out, plan(g_in), (None if symmetric else plan(g_out))


def _call(pin, pout, g_in, g_out, sources, delta, parents=True):
    n = g_in.num_rows
    dist, parent = (capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32)) for _ in range(2))
    win, wout = (capi.DeviceBuffer.from_host(g.adj_data if g.nnz else np.zeros(1, np.float32)) for g in (g_in, g_out))
    stats = pin.sssp_delta(pout, win, wout, sources, delta, dist, parent if parents else None)
    capi.sync()
    got = [b.read(np.uint32, n + 64) for b in (dist, parent)]
    assert all(np.all(g[n:] == GARBAGE) for g in got), "a guard word was written"
    assert parents or np.all(got[1] == GARBAGE)
    return got[0][:n], got[1][:n], stats


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_plans_no_sources_and_no_entries(gpu, n):
    ring = _csr(n, (np.arange(n) + 1) % n, np.arange(n), np.arange(1, n + 1)) if n > 1 else _csr(1, [], [], [])
    g_in, g_out, pin, pout = _plans(ring)
    want, parent, _ = dijkstra_f32(g_in, [n - 1, n - 1])            # (a source given twice counts once)
    dist, par, stats = _call(pin, pout, g_in, g_out, [n - 1, n - 1, n + 5], 2.0)
    assert np.array_equal(dist, bits(want)) and np.array_equal(par, parent) and stats[0] == n
    dist, par, stats = _call(pin, pout, g_in, g_out, [], 2.0)        # no sources: one launch, nobody reached
    assert np.all(dist == INF_BITS) and np.all(par == NONE) and stats == (0, 0, 0, 0, 1)
    empty = _csr(n, [], [], [])
    g_in, g_out, pin, pout = _plans(empty)
    dist, par, stats = _call(pin, pout, g_in, g_out, [0], np.inf, parents=False)
    assert dist[0] == 0 and np.all(dist[1:] == INF_BITS) and stats == (1, 0, 0, 0, 1)


@pytest.mark.gpu
def test_refusals(gpu):
    m = _case("grid_40")[0]
    g_in, g_out, pin, _ = _plans(m)
    path = _case("path_2000")[0]
    p_in, p_out, ppin, ppout = _plans(path)
    n = p_in.num_rows
    dist = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))
    w = capi.DeviceBuffer.from_host(p_in.adj_data)
    plan = lambda g, r0=0, r1=None: capi.SpMVPlan(g.num_rows, g.num_cols, g.adj_indptr, g.adj_indices, np.ones(g.nnz, np.float32), r0,
                                                   g.num_rows if r1 is None else r1, flags=capi.GL_PLAN_BOOLEAN)
    unsorted = io.CSRMatrix(1600, 1600, g_in.adj_data, g_in.adj_indices.copy(), g_in.adj_indptr)
    row = slice(int(g_in.adj_indptr[820]), int(g_in.adj_indptr[821]))
    unsorted.adj_indices[row] = unsorted.adj_indices[row][::-1]
    for a, b, code, needle in ((plan(unsorted), None, capi.GL_ERR_UNSUPPORTED, "strictly ascending"),
                               (ppin, ppin, capi.GL_ERR_UNSUPPORTED, "not symmetric"),
                               (ppin, pin, capi.GL_ERR_UNSUPPORTED, "not the transpose"),
                               (plan(p_in, 0, n // 2), ppout, capi.GL_ERR_UNSUPPORTED, "row shard")):
        with pytest.raises(capi.GraphLilyError) as e:
            a.sssp_delta(b, w, w, [0], 1.0, dist)
        assert e.value.code == code and needle in str(e.value) and "gl_sssp_delta" in str(e.value), str(e.value)
    for delta in (0.0, -1.0, np.nan):
        with pytest.raises(capi.GraphLilyError) as e:
            ppin.sssp_delta(ppout, w, w, [0], delta, dist)
        assert e.value.code == capi.GL_ERR_INVALID_ARG
        with pytest.raises(ValueError, match="delta"):
            _loaded("zero_cycle")[0].run(0, delta)
    assert np.all(dist.read(np.uint32, n) == GARBAGE), "a refused call writes nothing"
    for bad in (-1.0, np.nan, np.inf):
        d = app.ShortestPaths(M.num_hbm_channels, 1024, 256)
        with pytest.raises(ValueError, match=r"entry 1 \(2, 1\)"):
            d.load_and_format_matrix(_csr(8, [1, 2], [0, 1], [1, bad]), True)


@pytest.mark.gpu
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path):
    exe = build_cpp_driver("shortest_paths_driver.cpp")
    d, sources, ref = _loaded("grid_40")
    m = _case("grid_40")[0]
    path = str(tmp_path / "grid_40_csr_float32.npz")
    sp.save_npz(path, sp.csr_matrix((m.adj_data, m.adj_indices, m.adj_indptr), shape=(1600, 1600)), compressed=False)
    r = subprocess.run([exe, path, str(tmp_path), "1", "0", str(sources[0])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ShortestPaths::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_dist.bin"), dtype=np.uint32), bits(ref[0]))
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_parent.bin"), dtype=np.uint32), ref[1])
    assert "reached: %d\n" % int(np.isfinite(ref[0]).sum()) in r.stdout and "orphans: 0\n" in r.stdout
