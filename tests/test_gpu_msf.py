"""GPU parity of the minimum spanning forest (gl_msf, SpMVPlan.msf, SpMVModule.msf, app.MinimumSpanningForest,
graphlily::app::MinimumSpanningForest): every comparison is np.array_equal against a closed form or the host Kruskal of
tests/test_msf_cpu.py, which that file checks against networkx and scipy.  Under the order (key(w), lo, hi) the forest is unique: no
tolerance anywhere.  Output buffers start as garbage, every case is called twice on one plan, with and without d_labels, the labels
are compared with gl_cc_labels on the same plan, and forest edges + components == vertices."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import named_matrix, set_knob
from test_cc_cpu import permute_rows
from test_msf_cpu import (MSF_DRIVER, boruvka_rounds, build_cpp_driver, clique_edges, components_graph, entry_rows, graph_of, kruskal,
                          mask_of, ones_of, random_graph, raw_csr, special_graph, total_of)

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _msf(plan, weights, n, labels=True):
    """-> (forest words, labels or None, stats); the output buffers start out as garbage: the call writes every word itself"""
    nnz = weights.shape[0]
    w = capi.DeviceBuffer.from_host(np.ascontiguousarray(weights, np.float32))
    f = capi.DeviceBuffer.from_host(np.full(nnz, GARBAGE, np.uint32))
    lab = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32)) if labels else None
    stats = plan.msf(w, f, lab)
    capi.sync()
    assert len(stats) == 4 and 0xdeadbeefdeadbeef not in stats
    return f.read(np.uint32, nnz), (lab.read(np.uint32, n) if labels else None), stats


def _cc_labels(plan, n):
    out = capi.DeviceBuffer.from_host(np.full(n + 1, GARBAGE, np.uint32))
    plan.cc_labels(out, capi.DeviceBuffer(4, ptr=out.ptr + 4 * n, keepalive=out))
    capi.sync()
    got = out.read(np.uint32, n + 1)
    return got[:n], int(got[n])


def _check(sym, want, rounds=None, plan=None, weights=None):
    """the forest equals `want` (bool per entry), the labels equal gl_cc_labels', the stats describe the run; with and without
    d_labels on one plan"""
    n = sym.num_rows
    plan = _bool_plan(ones_of(sym)) if plan is None else plan
    weights = sym.adj_data if weights is None else weights
    want = np.asarray(want).astype(np.uint32)
    edges = int(want.sum()) // 2
    cc, components = _cc_labels(plan, n)
    forest, labels, stats = _msf(plan, weights, n)
    assert np.array_equal(forest, want) and np.array_equal(labels, cc)
    assert stats[0] + stats[1] == n and stats[:2] == (edges, components) and stats[3] >= 4
    if rounds is not None:
        assert stats[2] == rounds
    assert stats[2] <= max(n - 1, 0).bit_length()                          # ceil(log2 n)
    forest, labels, again = _msf(plan, weights, n, labels=False)
    assert np.array_equal(forest, want) and labels is None and again[:3] == stats[:3]
    return stats


@functools.lru_cache(maxsize=None)
def prepared(kind, seed=0):
    """-> (the matrix as given, its symmetric weighted form, Kruskal's mask, the synchronous round count); computed once, shared,
    never written"""
    if kind == "random":
        raw = random_graph(4096, 20000, seed)
    elif kind == "mid":
        raw = random_graph(1536, 9000, 40, top=5)
    else:
        raise KeyError(kind)
    sym = io.symmetrize_weighted(raw)[0]
    mask = kruskal(sym)
    mask.setflags(write=False)
    return raw, sym, mask, boruvka_rounds(sym)


def test_cycle_of_equal_weights(gpu):
    """C_200 on 5 .. 204, every weight 1: the forest is the cycle without its LAST edge in (lo, hi) order, (203, 204)"""
    v = np.arange(5, 205)
    g = graph_of(256, v, np.roll(v, -1), np.ones(200))
    want = mask_of(g, v[:-2].tolist() + [5], (v[:-2] + 1).tolist() + [204])
    assert int(want.sum()) == 2 * 199 and np.array_equal(want, kruskal(g))
    stats = _check(g, want, rounds=boruvka_rounds(g))
    assert stats[:2] == (199, 256 - 199)


@pytest.mark.parametrize("k", [3, 17, 65, 130])
def test_cliques_of_equal_weights(gpu, k):
    """K_k on 5 .. k + 4, every weight 1: the star at the smallest vertex, in one round -- every vertex chooses its edge to 5, and 5
    chooses (5, 6).  Rows of 64 and 129 entries cross the cut between a thread's and a wavefront's row."""
    a, b = clique_edges(k, 5)
    g = graph_of(256, a, b, np.ones(a.shape[0]))
    stats = _check(g, mask_of(g, np.full(k - 1, 5), np.arange(6, 5 + k)), rounds=1)
    assert stats[:2] == (k - 1, 256 - (k - 1))


def test_ascending_path_hangs_every_component_into_one_chain(gpu):
    """5000 vertices, w(i, i + 1) = i: vertex i > 0 chooses (i - 1, i), so ONE round takes every edge and leaves a chain of 4999
    hooks for the flatten"""
    i = np.arange(4999)
    g = graph_of(5120, i, i + 1, i)
    stats = _check(g, np.ones(g.nnz, bool), rounds=1)
    assert stats[:2] == (4999, 5120 - 4999)


def test_hierarchical_path_pairs_components_up(gpu):
    """1024 vertices, w(i, i + 1) = trailing zeros of i + 1: the components pair up in every round, ten rounds exactly"""
    i = np.arange(1023)
    tz = np.array([(int(x) & -int(x)).bit_length() - 1 for x in i + 1], dtype=np.float32)
    g = graph_of(1024, i, i + 1, tz)
    stats = _check(g, np.ones(g.nnz, bool), rounds=10)
    assert stats[:2] == (1023, 1)


def test_hubs(gpu):
    """a star with 5000 leaves, distinct and equal weights: one row of 5000 entries and 5000 far-side candidates for one word.  Then
    two hubs 0 and 1, both adjacent to the same 5000 leaves, and the edge (0, 1), heaviest and lightest"""
    leaves = np.arange(12, 5012)
    for w in (np.arange(5000)[::-1], np.ones(5000)):
        g = graph_of(5120, np.full(5000, 11), leaves, w)
        assert _check(g, np.ones(g.nnz, bool), rounds=1)[:2] == (5000, 120)
    leaves = np.arange(2, 5002)
    a, b = np.concatenate([[0], np.zeros(5000, np.int64), np.ones(5000, np.int64)]), np.concatenate([[1], leaves, leaves])
    g = graph_of(5120, a, b, np.concatenate([[2.0], np.ones(10000)]))            # (0, 1) heaviest: it closes a cycle
    want = mask_of(g, np.concatenate([np.zeros(5000, np.int64), [1]]), np.concatenate([leaves, [2]]))
    assert np.array_equal(want, kruskal(g))
    assert _check(g, want, rounds=boruvka_rounds(g))[:2] == (5001, 119)
    g = graph_of(5120, a, b, np.concatenate([[0.5], np.ones(10000)]))            # (0, 1) lightest: taken first
    want = mask_of(g, np.concatenate([[0], np.zeros(5000, np.int64)]), np.concatenate([[1], leaves]))
    assert np.array_equal(want, kruskal(g))
    assert _check(g, want, rounds=boruvka_rounds(g))[:2] == (5001, 119)
    rng = np.random.default_rng(17)                                               # and with distinct weights all over
    g = graph_of(5120, a, b, rng.permutation(10001))
    _check(g, kruskal(g), rounds=boruvka_rounds(g))


def test_special_values_and_mirror_words(gpu):
    """negative weights, +0.0, +-inf, 1e+-30 and subnormals in one graph: the order is by key.  Then the same graph with the words of
    the entries BELOW the diagonal set to NaN, and to -inf: bit-identical, the lower triangle is never read"""
    g = special_graph()
    want, rounds = kruskal(g), boruvka_rounds(g)
    plan = _bool_plan(ones_of(g))
    base = _check(g, want, rounds=rounds, plan=plan)
    below = g.adj_indices.astype(np.int64) < entry_rows(g)
    for word in (np.float32(np.nan), np.float32(-np.inf)):
        w = np.where(below, word, g.adj_data).astype(np.float32)
        assert _check(g, want, rounds=rounds, plan=plan, weights=w)[:3] == base[:3]
    w = g.adj_data.copy()                                      # -0.0 sorts below +0.0 at the C level
    zero = np.flatnonzero((w == 0) & ~below)
    w[zero[-1]] = np.float32(-0.0)
    h = io.CSRMatrix(g.num_rows, g.num_cols, w, g.adj_indices, g.adj_indptr)
    _check(h, kruskal(h), rounds=boruvka_rounds(h), plan=plan)


def test_components_isolated_and_padding_vertices(gpu):
    g = components_graph()
    stats = _check(g, kruskal(g), rounds=boruvka_rounds(g))
    assert stats[:2] == (8 + 59 + 129, 384 - (8 + 59 + 129))
    labels = _msf(_bool_plan(ones_of(g)), g.adj_data, 384)[1]
    assert np.all(labels[10:19] == 10) and np.all(labels[40:100] == 40) and np.all(labels[200:330] == 200)
    rest = np.setdiff1d(np.arange(384), np.concatenate([np.arange(10, 19), np.arange(40, 100), np.arange(200, 330)]))
    assert np.array_equal(labels[rest], rest)


def test_no_edges(gpu):
    n = 256
    e = raw_csr(n, [], [], [])                   # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    w = capi.DeviceBuffer.from_host(np.zeros(16, np.float32))
    out = capi.DeviceBuffer.from_host(np.full(16, GARBAGE, np.uint32))
    lab = capi.DeviceBuffer.from_host(np.full(n + 16, GARBAGE, np.uint32))
    for _ in range(2):
        assert empty.msf(w, out)[:3] == (0, n, 0)
        assert empty.msf(w, out, lab)[:3] == (0, n, 0)
    capi.sync()
    assert np.all(out.read(np.uint32, 16) == GARBAGE), "a plan without entries writes no forest words"
    got = lab.read(np.uint32, n + 16)
    assert np.array_equal(got[:n], np.arange(n)) and np.all(got[n:] == GARBAGE)
    none = capi.SpMVPlan(0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, 0, flags=capi.GL_PLAN_BOOLEAN)
    assert none.msf(w, out, lab) == (0, 0, 0, 0)
    only = raw_csr(128, [3, 9], [3, 9], [1.0, 1.0])                      # nothing but a diagonal: entries, and no edge
    forest, labels, stats = _msf(_bool_plan(only), only.adj_data, 128)
    assert not forest.any() and np.array_equal(labels, np.arange(128)) and stats[:3] == (0, 128, 0)
    msf = _driver(e)                                                      # the driver on a graph without edges
    assert msf.run(labels=True).shape == (0,) and msf.num_edges_ == 0 and msf.num_components_ == n and msf.total_weight_ == 0.0
    assert msf.edges_.shape == (0, 2) and np.array_equal(msf.labels_, np.arange(n))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_with_ties_everywhere(gpu, seed):
    """n = 4096, about 20 000 edges, integer weights 0 .. 7; the rows handed to the preparation in a random order"""
    raw, sym, want, rounds = prepared("random", seed)
    shuffled = io.symmetrize_weighted(permute_rows(raw, seed))[0]
    assert np.array_equal(shuffled.adj_indices, sym.adj_indices) and np.array_equal(shuffled.adj_data, sym.adj_data)
    _check(shuffled, want, rounds=rounds)


@pytest.mark.parametrize("knob,values", [("msf_batch", (1, 3)), ("msf_cut", (0, 8)), ("msf_grid", (1, 7)), ("msf_filter", (0, 1))])
def test_schedule_independence(gpu, monkeypatch, knob, values):
    """the rounds between two read-backs, the cut, the grid and the far-side filter change neither a bit of the result nor the
    rounds, which are a property of graph and weights; the knobs are read per call"""
    _, sym, want, rounds = prepared("mid")
    plan = _bool_plan(ones_of(sym))
    base = _check(sym, want, rounds=rounds, plan=plan)
    hubs = graph_of(5120, np.full(5000, 11), np.arange(12, 5012), np.arange(5000) % 7)
    for value in values:
        set_knob(monkeypatch, knob, value)
        assert _check(sym, want, rounds=rounds, plan=plan)[:3] == base[:3]
        _check(hubs, np.ones(hubs.nnz, bool), rounds=1)
    set_knob(monkeypatch, "msf_batch", 1)                                  # and batch 1 together with the knob's last setting
    assert _check(sym, want, rounds=rounds, plan=plan)[:3] == base[:3]


def test_refusals(gpu):
    _, sym, want, _ = prepared("mid")
    n, nnz = sym.num_rows, sym.nnz
    ones = ones_of(sym)
    plan = _bool_plan(ones)

    def still_works():
        forest, _, _ = _msf(plan, sym.adj_data, n, labels=False)
        assert np.array_equal(forest, want.astype(np.uint32))
    still_works()
    w = capi.DeviceBuffer.from_host(np.ones(nnz + 128, np.float32))
    out = capi.DeviceBuffer.from_host(np.full(nnz + 128, GARBAGE, np.uint32))
    lab = capi.DeviceBuffer.from_host(np.full(n + 128, GARBAGE, np.uint32))

    def refused(p, needle):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.msf(w, out, lab)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
            assert "gl_msf" in str(e.value)
        assert np.all(out.read(np.uint32, nnz + 128) == GARBAGE) and np.all(lab.read(np.uint32, n + 128) == GARBAGE), "a refused call writes nothing"
        still_works()
    general = capi.SpMVPlan(ones.num_rows, ones.num_cols, ones.adj_indptr, ones.adj_indices, ones.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "row copy")
    refused(_bool_plan(ones, 0, n // 2), "row shard")
    refused(_bool_plan(ones, n // 2, n), "row shard")
    sh = permute_rows(ones, 77)
    assert not np.array_equal(sh.adj_indices, ones.adj_indices)
    refused(_bool_plan(sh), "io.symmetrize_weighted")                      # unsorted rows
    wide = io.CSRMatrix(n, n + 128, ones.adj_data, ones.adj_indices, ones.adj_indptr)
    refused(_bool_plan(wide), "num_rows == num_cols")
    # one edge stored one way only: K_5 on 10 .. 14 in both directions, and (20, 21) without (21, 20)
    a, b = clique_edges(5, 10)
    one_way = raw_csr(256, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]]), np.ones(21))
    for needle in ("not symmetric", "io.symmetrize_weighted"):
        refused(_bool_plan(one_way), needle)
    zeros = io.CSRMatrix(n, n, sym.adj_data, sym.adj_indices, sym.adj_indptr)    # planned from the weights: a zero is stored as no entry
    assert np.any(sym.adj_data == 0)
    refused(_bool_plan(zeros), "strictly ascending sets")
    for args in ((None, out, lab), (w, None, lab), (w, out, out)):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.msf(*args)
        assert e.value.code == capi.GL_ERR_INVALID_ARG and "gl_msf" in str(e.value)
    assert capi.lib().gl_msf(None, ctypes.c_void_p(w.ptr), ctypes.c_void_p(out.ptr), None, None) == capi.GL_ERR_INVALID_ARG
    assert np.all(out.read(np.uint32, nnz + 128) == GARBAGE)
    still_works()


def _driver(m, weighted=True):
    msf = app.MinimumSpanningForest(M.num_hbm_channels, 1024, 256)
    msf.set_target("hw")
    msf.set_up_runtime("unused.xclbin")
    msf.load_and_format_matrix(m, True, weighted)
    msf.send_matrix_host_to_device()
    return msf


@functools.lru_cache(maxsize=None)
def weighted_uniform():
    """helpers.named_matrix("uniform_10K_10") with weights 0 .. 15 from a hash of the entry's ends (ties, and stored zeros)"""
    raw = named_matrix("uniform_10K_10")
    rows = np.repeat(np.arange(raw.num_rows, dtype=np.int64), np.diff(raw.adj_indptr.astype(np.int64)))
    cols = raw.adj_indices.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    raw.adj_data = ((lo * 2654435761 + hi * 40503) % 2**32 >> 7 & 15).astype(np.float32)
    return raw


@pytest.mark.parametrize("weighted", [True, False])
def test_drivers(gpu, weighted):
    raw = weighted_uniform()
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    sym = io.symmetrize_weighted(m, weighted)[0]
    want = kruskal(sym)
    msf = _driver(raw, weighted)
    got = msf.run(labels=True)
    assert got.dtype == bool and got.shape == (sym.nnz,) and msf.in_forest_ is got and msf.n_real_ == raw.num_rows
    assert np.array_equal(msf.graph_.adj_indices, sym.adj_indices) and np.array_equal(msf.graph_.adj_data, sym.adj_data)
    assert np.array_equal(got, want)
    assert app.validate_spanning_forest(raw, got, weighted) == msf.num_edges_ == int(want.sum()) // 2
    assert msf.total_weight_ == total_of(sym, want) and (weighted or msf.total_weight_ == msf.num_edges_)
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    once = want & (cols > rows)
    assert msf.edges_.shape == (msf.num_edges_, 2) and np.array_equal(msf.edges_[:, 0], rows[once]) and np.array_equal(msf.edges_[:, 1], cols[once])
    assert msf.weights_.dtype == np.float32 and np.array_equal(msf.weights_, sym.adj_data[once])
    labels = app._components_of(sym.adj_indptr, sym.adj_indices, None, sym.num_rows)
    assert msf.labels_.dtype == np.uint32 and np.array_equal(msf.labels_, labels)
    real = int(np.count_nonzero(labels[:raw.num_rows] == np.arange(raw.num_rows)))
    assert msf.num_components_ == real and msf.num_edges_ + real == raw.num_rows
    assert msf.rounds_ == boruvka_rounds(sym) and msf.launches_ >= 4
    assert np.array_equal(msf.run(), want) and msf.labels_ is None                 # a second run, without the labels
    assert np.array_equal(_driver(permute_rows(raw, 5), weighted).run(), want)     # the preparation sorts the rows


@pytest.mark.parametrize("weighted", [1, 0])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, weighted):
    import scipy.sparse as sp
    build_cpp_driver("msf_driver.cpp")
    raw = weighted_uniform()
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)                                            # (stored zeros stay stored)
    path = str(tmp_path / "uniform_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([MSF_DRIVER, path, str(tmp_path), str(weighted)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "MinimumSpanningForest::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    msf = _driver(raw, bool(weighted))
    want = msf.run(labels=True)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_forest.bin"), dtype=np.uint32), want.astype(np.uint32))
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_labels.bin"), dtype=np.uint32), msf.labels_)
    checksum = 0
    for c in want.astype(np.uint32).tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    assert "forest edges: %d\n" % msf.num_edges_ in r.stdout and "components: %d\n" % msf.num_components_ in r.stdout
    assert "rounds: %d\n" % msf.rounds_ in r.stdout and "total weight: %.17g\n" % msf.total_weight_ in r.stdout
    assert "checksum: %d\n" % checksum in r.stdout
