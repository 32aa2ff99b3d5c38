"""GPU parity of the greedy weighted matching (gl_match, SpMVPlan.match, SpMVModule.match, app.Matching, graphlily::app::Matching):
every comparison is np.array_equal against the host greedy() of tests/test_match_cpu.py, and rounds and scans equal those of its
pointer_rounds(); that file checks both against each other, closed forms and networkx.  Under the order (~key(w), lo, hi) the
matching is unique: no tolerance anywhere.  The output buffer starts as garbage and every case is called twice on one plan."""
import ctypes
import functools
import subprocess
import time

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import named_matrix, set_knob
from test_cc_cpu import permute_rows
from test_msf_cpu import clique_edges, entry_rows, graph_of, ones_of, raw_csr
from test_match_cpu import (FREE, MATCH_DRIVER, build_cpp_driver, gpu_graph, greedy, mate_of_pairs, pairs_of, pointer_rounds, weight_of)

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef


@pytest.fixture(autouse=True, params=[None, 0], ids=["spread", "thread_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of a list to the wavefronts -- these graphs are small, so their lists are
    spread, a row per wavefront (the driver tests' round 1: two) -- and with match_spread=0, which keeps 64 rows per wavefront,
    a thread per row up to the cut"""
    set_knob(monkeypatch, "match_spread", request.param)


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _match(plan, weights, n):
    """-> (mates, stats); the output buffer starts out as garbage, and a guard behind it must stay garbage"""
    w = capi.DeviceBuffer.from_host(np.ascontiguousarray(weights, np.float32))
    out = capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32))
    stats = plan.match(w, out)
    capi.sync()
    got = out.read(np.uint32, n + 64)
    assert len(stats) == 4 and 0xdeadbeefdeadbeef not in stats and np.all(got[n:] == GARBAGE)
    return got[:n], stats


def _check(sym, want, rounds, scans, plan=None, weights=None):
    """the mates equal `want`, the stats are the host model's; twice on one plan"""
    n = sym.num_rows
    plan = _bool_plan(ones_of(sym)) if plan is None else plan
    weights = sym.adj_data if weights is None else weights
    mate, stats = _match(plan, weights, n)
    assert np.array_equal(mate, want)
    assert stats[:3] == (len(pairs_of(want)), rounds, scans) and stats[3] >= 7
    mate, again = _match(plan, weights, n)
    assert np.array_equal(mate, want) and again == stats
    return stats


def _check_named(name, **kw):
    sym, want, rounds, scans = gpu_graph(name)
    return _check(sym, want, rounds, scans, **kw)


@pytest.mark.parametrize("name", ["path_ascending", "path_equal"])
def test_paths_match_one_pair_per_round(gpu, name):
    """600 of 640 vertices: with w = i the heaviest edge is the last one and (598, 599), (596, 597), ... follow one round apart;
    with equal weights (0, 1), (2, 3), ... do: the dependency chain runs across many gated batches"""
    lo = np.arange(0, 600, 2)
    sym, want, rounds, scans = gpu_graph(name)
    assert np.array_equal(want, mate_of_pairs(640, lo, lo + 1)) and rounds == 300 and scans == 600 + 299
    stats = _check_named(name)
    assert stats[0] == 300 and np.all(want[600:] == FREE)


@pytest.mark.parametrize("k", [3, 17, 65, 130])
def test_cliques_of_equal_weights(gpu, k):
    """K_k on 5 .. k + 4, every weight 1: (5, 6), (7, 8), ... one pair per round, and every free vertex rescans every round.  Rows
    of 64 and 129 entries cross the cut between a thread's and a wavefront's row."""
    sym, want, rounds, scans = gpu_graph("clique_%d" % k)
    lo = 5 + np.arange(0, k - 1, 2)
    assert np.array_equal(want, mate_of_pairs(256, lo, lo + 1)) and rounds == (k + 1) // 2
    assert _check_named("clique_%d" % k)[0] == k // 2


@pytest.mark.parametrize("name", ["star_distinct", "star_equal"])
def test_star(gpu, name):
    """a star with 5000 leaves: one row of 5000 entries, and one fresh vertex that hands 4999 vertices to the next list"""
    sym, want, rounds, scans = gpu_graph(name)
    assert np.array_equal(want, mate_of_pairs(5120, [11], [12])) and (rounds, scans) == (2, 10000)
    _check_named(name)


@pytest.mark.parametrize("name", ["hubs_heaviest", "hubs_lightest"])
def test_two_hubs(gpu, name):
    """two hubs 0 and 1 over the same 5000 leaves and the edge (0, 1): heaviest, it is the matching; lightest, (0, 2) and (1, 3) are"""
    want = gpu_graph(name)[1]
    assert pairs_of(want) == ({(0, 1)} if name == "hubs_heaviest" else {(0, 2), (1, 3)})
    _check_named(name)


def test_special_values(gpu):
    """negative weights, +0.0, +-inf, 1e+-30 and subnormals over K_24: the order is by key.  -0.0 sorts below +0.0 at the C level,
    and the driver turns a -0.0 of the raw matrix into +0.0"""
    sym, want, rounds, scans = gpu_graph("special")
    plan = _bool_plan(ones_of(sym))
    _check(sym, want, rounds, scans, plan=plan)
    w = sym.adj_data.copy()                                    # both entries of one zero-weight edge become -0.0
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    j = int(np.flatnonzero((w == 0) & (cols > rows))[-1])
    w[j] = w[int(np.flatnonzero((rows == cols[j]) & (cols == rows[j]))[0])] = np.float32(-0.0)
    h = io.CSRMatrix(sym.num_rows, sym.num_cols, w, sym.adj_indices, sym.adj_indptr)
    mate, r, s = pointer_rounds(h)
    assert np.array_equal(mate, greedy(h))
    _check(h, mate, r, s, plan=plan)
    raw = raw_csr(128, [0, 1, 2], [1, 2, 3], [-0.0, 0.0, -1.0])             # -0.0 == +0.0 after the preparation: (0, 1) first
    d = _driver(raw)
    assert pairs_of(d.run()) == {(0, 1), (2, 3)} and not np.any(np.signbit(d.graph_.adj_data) & (d.graph_.adj_data == 0))
    sym0 = graph_of(128, [0, 1, 2], [1, 2, 3], [-0.0, 0.0, -1.0])
    w = sym0.adj_data.copy()
    w[:2] = np.float32(-0.0)                                                # at the C level (0, 1) = -0.0 < (1, 2) = +0.0
    mate, _ = _match(_bool_plan(ones_of(sym0)), w, 128)
    assert pairs_of(mate) == {(1, 2)}


def test_components_isolated_and_padding_vertices(gpu):
    sym, want, rounds, scans = gpu_graph("components")
    _check(sym, want, rounds, scans)
    rest = np.setdiff1d(np.arange(384), np.concatenate([np.arange(10, 19), np.arange(40, 100), np.arange(200, 330)]))
    assert np.all(want[rest] == FREE)


def test_no_edges(gpu):
    n = 256
    e = raw_csr(n, [], [], [])                   # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        mate, stats = _match(empty, np.zeros(16, np.float32), n)
        assert np.all(mate == FREE) and stats == (0, 0, 0, 1)
    none = capi.SpMVPlan(0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, 0, flags=capi.GL_PLAN_BOOLEAN)
    assert _match(none, np.zeros(16, np.float32), 0)[1] == (0, 0, 0, 0)
    only = raw_csr(128, [3, 9], [3, 9], [1.0, 1.0])                      # nothing but a diagonal: two rows to scan, and no edge
    mate, stats = _match(_bool_plan(only), only.adj_data, 128)
    assert np.all(mate == FREE) and stats[:3] == (0, 1, 2)
    d = _driver(e)                                                        # the driver on a graph without edges
    assert np.all(d.run() == FREE) and d.mate_.shape == (n,) and d.num_matched_ == 0 and d.total_weight_ == 0.0
    assert d.edges_.shape == (0, 2) and d.in_matching_.shape == (0,) and (d.rounds_, d.scans_) == (0, 0)


@pytest.mark.parametrize("name", ["random_1", "random_2", "mid", "mid_distinct", "wide"])
def test_random_with_ties_everywhere(gpu, name):
    """n = 4096 with about 20 000 edges of integer weights 0 .. 7, n = 1536 with 9000 edges of weights 0 .. 4, and a copy of that
    with all-distinct weights; n = 40 960 with about 100 000 edges, whose first lists are spread eight and four rows to a wavefront"""
    _check_named(name)


@pytest.mark.parametrize("knob,values", [("match_batch", (1, 64)), ("match_cut", (0,)), ("match_grid", (1, 7)), ("match_spread", (1, 32))])
def test_schedule_independence(gpu, monkeypatch, knob, values):
    """the rounds between two read-backs, the cut, the grid and how a short list is spread over the wavefronts change neither a bit of the result nor rounds and scans, which are
    properties of graph and weights; the knobs are read per call"""
    sym, want, rounds, scans = gpu_graph("mid")
    plan = _bool_plan(ones_of(sym))
    base = _check(sym, want, rounds, scans, plan=plan)
    for value in values:
        set_knob(monkeypatch, knob, value)
        assert _check(sym, want, rounds, scans, plan=plan)[:3] == base[:3]
        _check_named("clique_130")
        _check_named("star_equal")
    set_knob(monkeypatch, "match_batch", 1)                               # and batch 1 together with the knob's last setting
    assert _check(sym, want, rounds, scans, plan=plan)[:3] == base[:3]
    _check_named("path_equal")


def test_refusals(gpu):
    sym, want, rounds, scans = gpu_graph("mid")
    n, nnz = sym.num_rows, sym.nnz
    ones = ones_of(sym)
    plan = _bool_plan(ones)

    def still_works():
        assert np.array_equal(_match(plan, sym.adj_data, n)[0], want)
    still_works()
    w = capi.DeviceBuffer.from_host(np.ones(nnz + 128, np.float32))
    out = capi.DeviceBuffer.from_host(np.full(n + 128, GARBAGE, np.uint32))

    def refused(p, needle):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.match(w, out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
            assert "gl_match" in str(e.value)
        assert np.all(out.read(np.uint32, n + 128) == GARBAGE), "a refused call writes nothing"
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
    for args in ((None, out), (w, None)):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.match(*args)
        assert e.value.code == capi.GL_ERR_INVALID_ARG and "gl_match" in str(e.value)
    assert capi.lib().gl_match(None, ctypes.c_void_p(w.ptr), ctypes.c_void_p(out.ptr), None) == capi.GL_ERR_INVALID_ARG
    assert np.all(out.read(np.uint32, n + 128) == GARBAGE)
    still_works()


def test_mirrored_weights_that_differ_are_refused_promptly(gpu):
    """a triangle whose entries say 0 prefers 1, 1 prefers 2 and 2 prefers 0: the pointers close a cycle, no pair can form, and the
    call says so instead of hanging or returning a matching that is not maximal.  The plan works afterwards."""
    tri = graph_of(128, [0, 1, 0], [1, 2, 2], [1.0, 1.0, 1.0])
    assert tri.adj_indices.tolist() == [1, 2, 0, 2, 0, 1]
    #               (0,1) (0,2) (1,0) (1,2) (2,0) (2,1)
    w = np.array([3.0, 1.0, 1.0, 3.0, 3.0, 1.0], np.float32)
    plan = _bool_plan(ones_of(tri))
    wb = capi.DeviceBuffer.from_host(w)
    out = capi.DeviceBuffer.from_host(np.full(128, GARBAGE, np.uint32))
    t0 = time.perf_counter()
    for _ in range(2):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.match(wb, out)
        assert e.value.code == capi.GL_ERR_INVALID_ARG and "different weight bits" in str(e.value) and "gl_match" in str(e.value)
    assert time.perf_counter() - t0 < 5.0
    mate, stats = _match(plan, tri.adj_data, 128)
    assert pairs_of(mate) == {(0, 1)} and stats[:3] == (1, 2, 4)


def _driver(m, weighted=True, drop_nonpositive=False):
    d = app.Matching(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True, weighted, drop_nonpositive)
    d.send_matrix_host_to_device()
    return d


@functools.lru_cache(maxsize=None)
def weighted_uniform():
    """helpers.named_matrix("uniform_10K_10") with weights -3 .. 12 from a hash of the entry's ends (ties, stored zeros, negatives)"""
    raw = named_matrix("uniform_10K_10")
    rows = np.repeat(np.arange(raw.num_rows, dtype=np.int64), np.diff(raw.adj_indptr.astype(np.int64)))
    cols = raw.adj_indices.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    raw.adj_data = ((lo * 2654435761 + hi * 40503) % 2**32 >> 7 & 15).astype(np.float32) - 3.0
    return raw


@pytest.mark.parametrize("weighted,drop", [(True, False), (True, True), (False, False)])
def test_drivers(gpu, weighted, drop):
    raw = weighted_uniform()
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    sym = app._matching_graph_of(m, weighted, drop)[0]
    assert (not drop or np.all(sym.adj_data > 0)) and (weighted or np.all(sym.adj_data == 1))
    want, rounds, scans = pointer_rounds(sym)
    assert np.array_equal(want, greedy(sym))
    d = _driver(raw, weighted, drop)
    got = d.run()
    assert got.dtype == np.uint32 and got.shape == (sym.num_rows,) and d.mate_ is got and d.n_real_ == raw.num_rows
    assert np.array_equal(d.graph_.adj_indices, sym.adj_indices) and np.array_equal(d.graph_.adj_data, sym.adj_data)
    assert np.array_equal(got, want)
    # the plan-level call on the same graph
    assert np.array_equal(_match(_bool_plan(ones_of(sym)), sym.adj_data, sym.num_rows)[0], got)
    pairs = sorted(pairs_of(want))
    assert app.validate_matching(m, got, weighted, drop) == d.num_matched_ == len(pairs)      # (m: the padded matrix, n_ vertices)
    assert (d.rounds_, d.scans_) == (rounds, scans) and d.launches_ >= 7
    assert d.edges_.dtype == np.int64 and d.edges_.shape == (len(pairs), 2) and [tuple(e) for e in d.edges_.tolist()] == pairs
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    marked = want.astype(np.int64)[rows] == cols
    assert d.in_matching_.dtype == bool and np.array_equal(d.in_matching_, marked) and int(marked.sum()) == 2 * len(pairs)
    assert d.weights_.dtype == np.float32 and np.array_equal(d.weights_, sym.adj_data[marked & (cols > rows)])
    assert d.total_weight_ == weight_of(sym, want) and (weighted or d.total_weight_ == d.num_matched_)
    assert np.array_equal(d.run(), want)                                           # a second run
    assert np.array_equal(_driver(permute_rows(raw, 5), weighted, drop).run(), want)     # the preparation sorts the rows


@pytest.mark.parametrize("weighted,drop", [(1, 0), (1, 1), (0, 0)])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, weighted, drop):
    import scipy.sparse as sp
    build_cpp_driver("match_driver.cpp")
    raw = weighted_uniform()
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)                                            # (stored zeros stay stored)
    path = str(tmp_path / "uniform_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([MATCH_DRIVER, path, str(tmp_path), str(weighted), str(drop)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Matching::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(raw, bool(weighted), bool(drop))
    want = d.run()
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_mate.bin"), dtype=np.uint32), want)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    assert "matched edges: %d\n" % d.num_matched_ in r.stdout and "rounds: %d\n" % d.rounds_ in r.stdout
    assert "scans: %d\n" % d.scans_ in r.stdout and "total weight: %.17g\n" % d.total_weight_ in r.stdout
    assert "checksum: %d\n" % checksum in r.stdout
