"""GPU parity of the k-core decomposition (gl_kcore, SpMVPlan.kcore, SpMVModule.kcore, app.KCore, graphlily::app::KCore): every
comparison of core numbers is np.array_equal against the host definition (tests/test_kcore_cpu.py) or a closed form; an order is
not unique, so it is checked by its properties (app.validate_cores, rule 3).  The definition is exact: no tolerance anywhere."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_cc_cpu import permute_rows
from test_kcore_cpu import KCORE_DRIVER, RECORDS, SUB_ROUNDS, _csr, build_cpp_driver, core_numbers_by_peeling, prepared

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef


@functools.lru_cache(maxsize=None)
def _reference(name):
    """-> (the matrix as given, padded, symmetric form, core numbers of the padded matrix's vertices); shared, never written.
    On the two larger graphs the one-vertex-at-a-time host peel takes four to five seconds, so their reference is the validator's
    set peel, PROVEN right here: every v has at least core[v] neighbours u with core[u] >= core[v] (rule 1 of validate_cores: v
    then lies in a subgraph of minimum degree core[v], so no value is too high) and the sum is the recorded one (cross-checked
    against networkx: test_kcore_cpu.RECORDS), so no value is too low either.  The set peel is thus used as a fast way to a
    candidate, and what makes the candidate the reference is that argument, not the peel."""
    if name in ("rmat_sym_50K", "gplus_small"):
        from helpers import named_matrix
        raw = named_matrix(name)
        m = raw.copy()
        io.util_round_csr_matrix_dim(m, 128, 128)
        sym, _ = io.symmetrize_simple(m)
        core = app._core_numbers_of(sym.adj_indptr, sym.adj_indices, sym.num_rows).astype(np.uint32)
        assert app.validate_cores(m, core) == RECORDS[name][0] and int(core.sum()) == RECORDS[name][1]
        core.setflags(write=False)
        return raw, m, sym, core
    return prepared(name)[:4]


def _driver(m):
    kc = app.KCore(M.num_hbm_channels, 1024, 256)
    kc.set_target("hw")
    kc.set_up_runtime("unused.xclbin")
    kc.load_and_format_matrix(m, True)
    kc.send_matrix_host_to_device()
    return kc


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _kcore(plan, n, order=True):
    """-> (core, order or None, stats); the buffers start out as garbage: the call writes every word itself"""
    core = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))
    ordr = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32)) if order else None
    stats = plan.kcore(core, ordr)
    assert len(stats) == 4 and GARBAGE not in stats[:3]
    return core.read(np.uint32, n), (ordr.read(np.uint32, n) if order else None), stats


def _graph(n, a, b):
    """the undirected simple graph with the edges {a[i], b[i]} on n vertices, as gl_kcore wants it"""
    return io.symmetrize_simple(_csr(n, a, b))[0]


def _sorted_rows(m):
    """the columns of every row ascending (every value is 1)"""
    rows = np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64)))
    m.adj_indices = m.adj_indices[np.lexsort((m.adj_indices, rows))]
    return m


def _check(sym, want, sub_rounds=None):
    """core numbers equal `want`, the order is a degeneracy ordering, the stats describe the run; twice on one plan"""
    n = sym.num_rows
    plan = _bool_plan(sym)
    want = np.asarray(want, np.uint32)
    for _ in range(2):                                               # (the second time from the cached verdicts)
        core, order, stats = _kcore(plan, n)
        assert np.array_equal(core, want)
        assert app.validate_cores(sym, core, order) == int(want.max())
        assert stats[0] == int(want.max()) and stats[1] == np.unique(want).shape[0]
        if sub_rounds is not None:
            assert stats[2] == sub_rounds
    core, order, stats2 = _kcore(plan, n, order=False)
    assert np.array_equal(core, want) and order is None and stats2[:3] == stats[:3]
    return stats


@pytest.mark.parametrize("name", ["uniform_10K_10", "rmat_20K", "rmat_sym_50K", "gplus_small", "line_8", "eye_10", "many"])
def test_drivers(gpu, name):
    raw, m, sym, want = _reference(name)
    kc = _driver(raw)
    got = kc.run(order=True)
    assert got.dtype == np.uint32 and got.shape == (m.num_rows,) and kc.n_real_ == raw.num_rows and kc.core_ is got
    assert np.array_equal(got, want)
    assert kc.order_.dtype == np.uint32 and app.validate_cores(m, got, kc.order_) == kc.degeneracy_ == int(want.max())
    if name in RECORDS:
        assert (kc.degeneracy_, int(got.sum())) == RECORDS[name]
        assert kc.sub_rounds_ == SUB_ROUNDS[name]                    # a property of the graph: pins the schedule
    assert not got[raw.num_rows:].any()
    assert np.array_equal(kc.degrees_, np.diff(sym.adj_indptr.astype(np.int64)))
    if sym.nnz:
        assert kc.levels_ == np.unique(want).shape[0] and 1 <= kc.sub_rounds_ <= m.num_rows and kc.launches_ >= 1 + 3 * kc.sub_rounds_
    else:                                                            # (eye_10: an empty graph, nothing is launched)
        assert (kc.levels_, kc.sub_rounds_, kc.launches_) == (0, 0, 0)
    real = want[:raw.num_rows]
    assert kc.core_sizes_.shape == (kc.degeneracy_ + 1,) and kc.core_sizes_[0] == raw.num_rows
    assert all(kc.core_sizes_[k] == np.count_nonzero(real >= k) for k in range(kc.degeneracy_ + 1))
    top = kc.k_core(kc.degeneracy_)
    assert top.dtype == bool and top.shape == (m.num_rows,) and np.array_equal(np.flatnonzero(top), np.flatnonzero(real == kc.degeneracy_))
    assert np.count_nonzero(kc.k_core(0)) == raw.num_rows and not kc.k_core(kc.degeneracy_ + 1).any()
    sub = kc.sub_rounds_
    assert np.array_equal(kc.run(), want) and kc.order_ is None and kc.sub_rounds_ == sub      # a second run, without the order


@pytest.mark.parametrize("name", ["uniform_10K_10", "rmat_20K"])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, name):
    import scipy.sparse as sp
    build_cpp_driver("kcore_driver.cpp")
    raw, m, sym, want = _reference(name)
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / (name + "_csr_float32.npz"))
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([KCORE_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "KCore::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "cpp_core.bin"), dtype=np.uint32)
    assert np.array_equal(got, want)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    assert "degeneracy: %d\n" % RECORDS[name][0] in r.stdout and "sum of core numbers: %d\n" % RECORDS[name][1] in r.stdout
    assert "checksum: %d\n" % checksum in r.stdout
    assert "levels: %d\n" % np.unique(want).shape[0] in r.stdout


def _clique_edges(k, first):
    iu = np.triu_indices(k, 1)
    return iu[0] + first, iu[1] + first


@pytest.mark.parametrize("k", [2, 3, 5, 9, 10, 33, 34, 65, 66, 258])
def test_cliques_across_the_step_the_cut_and_the_takeover(gpu, k):
    """K_k on the vertices 5 .. k + 4: rows of k - 1 entries -- within one 4-entry step, across the cut (8 entries by default, 32
    with the knob of the test below), the wavefront (64) and the 256-entry takeover step -- behind k - 1 levels that find nobody but the isolated vertices of level 0"""
    n = 256 if k <= 66 else 512
    want = np.zeros(n, np.uint32)
    want[5:5 + k] = k - 1
    a, b = _clique_edges(k, 5)
    # one sub-round, over the isolated vertices of level 0: the scan of level k - 1 queues the whole clique, the queue then holds
    # every vertex and the run is over (the last slice has only queued neighbours: it is never peeled)
    _check(_graph(n, a, b), want, sub_rounds=1)


def test_path_longer_than_any_batch(gpu):
    """600 vertices in a row: core 1, peeled from both ends, two vertices per sub-round -- 299 sub-rounds inside ONE level (the
    300th slice, the two middle vertices, completes the queue and is not peeled) and one over the isolated vertices of level 0:
    more than a batch enqueues, so the gating carries the level across batches"""
    n, first = 1024, 7
    v = np.arange(first, first + 600)
    want = np.zeros(n, np.uint32)
    want[v] = 1
    stats = _check(_graph(n, v[:-1], v[1:]), want, sub_rounds=300)
    assert stats[3] >= 1 + 3 * (300 + 2)                             # two scans
    rng = np.random.default_rng(5)                                   # the same path under shuffled vertex numbers
    p = rng.permutation(n)
    _check(_graph(n, p[v[:-1]], p[v[1:]]), want[np.argsort(p)], sub_rounds=300)


def test_cycle_star_and_tree(gpu):
    n, first = 640, 3
    v = np.arange(first, first + 500)
    want = np.zeros(n, np.uint32)
    want[v] = 2
    _check(_graph(n, v, np.roll(v, -1)), want, sub_rounds=1)
    # a star with 5000 leaves: 5000 concurrent decrements of one word; the hub is appended once (the order is a permutation)
    n, hub = 5120, 11
    leaves = np.arange(hub + 1, hub + 5001)
    want = np.zeros(n, np.uint32)
    want[hub:hub + 5001] = 1
    _check(_graph(n, np.full(5000, hub), leaves), want, sub_rounds=2)            # level 0, the leaves
    # a complete binary tree of 2047 vertices: the leaves, then their parents ... one generation per sub-round
    n, first = 2176, 9
    child = np.arange(1, 2047)
    want = np.zeros(n, np.uint32)
    want[first:first + 2047] = 1
    _check(_graph(n, (child - 1) // 2 + first, child + first), want)


def test_cliques_joined_by_a_path_and_pendant_vertices(gpu):
    # K_20 on 4 .. 23, K_50 on 24 .. 73, a path 23 - 74 - 75 - ... - 85 - 24 between them and a path 86 - ... - 95 hanging off 85.
    # The joining path's inner vertices have degree 2 and both its ends are held by a clique, so cliques and path together have
    # minimum degree 2: those vertices have core number 2, not 1 (the host peel and networkx agree); the hanging path has 1.
    # (The issue's closed form for this case reads 19 / 49 / 1: it is 19 / 49 / 2 for the joining path, and the hanging path is
    # added so that core number 1 next to the cliques is still covered.)
    n = 256
    a1, b1 = _clique_edges(20, 4)
    a2, b2 = _clique_edges(50, 24)
    chain = np.concatenate([[23], np.arange(74, 86), [24]])
    tail = np.arange(85, 96)
    want = np.zeros(n, np.uint32)
    want[4:24], want[24:74], want[74:86], want[86:96] = 19, 49, 2, 1
    g = _graph(n, np.concatenate([a1, a2, chain[:-1], tail[:-1]]), np.concatenate([b1, b2, chain[1:], tail[1:]]))
    assert np.array_equal(core_numbers_by_peeling(g)[0], want)
    _check(g, want)
    # K_40 on 6 .. 45 with a pendant vertex on every member (and three on the first)
    n = 384
    a, b = _clique_edges(40, 6)
    pend = np.arange(100, 140)
    want = np.zeros(n, np.uint32)
    want[6:46], want[100:140], want[200:203] = 39, 1, 1
    _check(_graph(n, np.concatenate([a, np.arange(6, 46), [6, 6, 6]]), np.concatenate([b, pend, [200, 201, 202]])), want)


@pytest.mark.parametrize("cut", [0, 4, 32])
@pytest.mark.parametrize("batch", [1, 2, 64])
def test_knobs_change_neither_the_cores_nor_the_sub_rounds(gpu, monkeypatch, cut, batch):
    """sub-rounds are a property of the graph: neither where the wavefront takes a row over nor how many launches are enqueued
    between two read-backs of the control record changes them; the knobs are read per call"""
    _, m, sym, want = _reference("rmat_20K")
    n = sym.num_rows
    plan = _bool_plan(sym)
    _, _, base = _kcore(plan, n)
    v = np.arange(7, 607)
    path = _graph(1024, v[:-1], v[1:])
    path_plan = _bool_plan(path)
    path_want = np.zeros(1024, np.uint32)
    path_want[v] = 1
    set_knob(monkeypatch, "kcore_cut", cut)
    set_knob(monkeypatch, "kcore_batch", batch)
    core, order, stats = _kcore(plan, n)
    assert np.array_equal(core, want) and stats[:3] == base[:3] and stats[0] == RECORDS["rmat_20K"][0]
    assert app.validate_cores(sym, core, order) == stats[0]
    assert (stats[3] - 1) % (3 * batch) == 0
    core, order, stats = _kcore(path_plan, 1024)
    assert np.array_equal(core, path_want) and stats[:3] == (1, 2, 300)
    assert app.validate_cores(path, core, order) == 1


def test_entry_list_with_a_nonzero_first_offset(gpu):
    """the C ABI accepts a whole-matrix CSR whose indptr[0] is k != 0: the row copy's offsets then count from the caller's entry
    list while its indices start at entry k (csr_nz_base)"""
    _, m, sym, want = _reference("uniform_10K_10")
    n, k = sym.num_rows, 77
    junk = np.full(k, n - 1, np.uint32)                              # (entries in front of row 0 that belong to no row)
    plan = capi.SpMVPlan(n, n, sym.adj_indptr + np.uint32(k), np.concatenate([junk, sym.adj_indices]),
                         np.concatenate([np.ones(k, np.float32), sym.adj_data]), 0, n, flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean" and plan.info()["nnz"] == sym.nnz
    for _ in range(2):
        core, order, stats = _kcore(plan, n)
        assert np.array_equal(core, want) and app.validate_cores(sym, core, order) == RECORDS["uniform_10K_10"][0]
    # hub rows through the wavefront's takeover: the star's row of 5000 entries and K_200
    a, b = _clique_edges(200, 1)
    g = _graph(5120, np.concatenate([np.zeros(5000, np.int64), a]), np.concatenate([np.arange(1, 5001), b]))
    gw, _ = core_numbers_by_peeling(g)
    assert gw[0] == 200 and gw[200] == 200 and gw[201] == 1
    plan = capi.SpMVPlan(5120, 5120, g.adj_indptr + np.uint32(k), np.concatenate([junk * 0, g.adj_indices]),
                         np.concatenate([np.ones(k, np.float32), g.adj_data]), 0, 5120, flags=capi.GL_PLAN_BOOLEAN)
    core, order, stats = _kcore(plan, 5120)
    assert np.array_equal(core, gw) and app.validate_cores(g, core, order) == 200


def test_empty_plan_and_a_diagonal(gpu):
    n = 256
    e = _csr(n, [], [])                          # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        core, order, stats = _kcore(empty, n)
        assert not core.any() and np.array_equal(order, np.arange(n, dtype=np.uint32)) and stats == (0, 0, 0, 0)
    core, order, stats = _kcore(empty, n, order=False)
    assert not core.any() and stats == (0, 0, 0, 0)
    # the ABI ignores an entry (v, v): a triangle 3 - 4 - 5 with a diagonal entry on 3, on 4 and on the isolated vertex 9
    a, b = np.array([3, 4, 5, 3, 4, 5, 3, 4, 9]), np.array([4, 5, 3, 5, 3, 4, 3, 4, 9])
    d = _sorted_rows(_csr(n, a, b))
    want = np.zeros(n, np.uint32)
    want[3:6] = 2
    core, order, stats = _kcore(_bool_plan(d), n)
    assert np.array_equal(core, want) and app.validate_cores(d, core, order) == 2 and stats[:2] == (2, 2)


def test_refusals(gpu):
    _, m, sym, want = _reference("uniform_10K_10")
    n = sym.num_rows
    plan = _bool_plan(sym)

    def still_works():
        core, order, stats = _kcore(plan, n)
        assert np.array_equal(core, want) and stats[0] == RECORDS["uniform_10K_10"][0]
    still_works()
    out = capi.DeviceBuffer.from_host(np.full(n + 128, GARBAGE, np.uint32))
    word = capi.DeviceBuffer(8)
    labels = capi.DeviceBuffer(4 * (n + 128))

    def refused(p, needle, tc_total=None, components=None):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.kcore(out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
        assert np.all(out.read(np.uint32, n + 128) == GARBAGE), "a refused call writes nothing"
        # the plan is still usable for what it does support
        if tc_total is not None:
            p.tc_count(word)
            capi.sync()
            assert int(word.read(np.uint64, 1)[0]) == tc_total
        if components is not None:
            p.cc_labels(labels, word)
            capi.sync()
            assert int(word.read(np.uint32, 1)[0]) == components
        still_works()
    general = capi.SpMVPlan(sym.num_rows, sym.num_cols, sym.adj_indptr, sym.adj_indices, sym.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "row copy")
    refused(_bool_plan(sym, 0, n // 2), "row shard")
    refused(_bool_plan(sym, n // 2, n), "row shard")
    ncomp = app.validate_components(sym, app._components_of(sym.adj_indptr, sym.adj_indices, None, n))
    sh = permute_rows(sym, 77)
    assert not np.array_equal(sh.adj_indices, sym.adj_indices)
    refused(_bool_plan(sh), "io.symmetrize_simple", components=ncomp)
    z = sym.copy()
    z.adj_data[np.random.default_rng(2).random(z.nnz) < 0.01] = 0.0
    assert np.any(z.adj_data == 0)
    refused(_bool_plan(z), "strictly ascending")
    wide = io.CSRMatrix(n, n + 128, sym.adj_data, sym.adj_indices, sym.adj_indptr)
    refused(_bool_plan(wide), "num_rows == num_cols", components=ncomp + 128)
    # one edge stored one way only: K_5 on 10 .. 14 in both directions, and (20, 21) without (21, 20)
    a, b = _clique_edges(5, 10)
    one_way = _sorted_rows(_csr(256, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]])))
    refused(_bool_plan(one_way), "not symmetric", tc_total=60, components=256 - 4 - 1)
    # with the edge's other copy the same graph is accepted
    both = _graph(256, np.concatenate([a, [20]]), np.concatenate([b, [21]]))
    core, _, _ = _kcore(_bool_plan(both), 256)
    assert core[10:15].tolist() == [4] * 5 and core[20] == core[21] == 1 and int(core.sum()) == 22
    with pytest.raises(capi.GraphLilyError) as e:
        plan.kcore(None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    with pytest.raises(capi.GraphLilyError) as e:
        plan.kcore(out, out)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    assert capi.lib().gl_kcore(None, ctypes.c_void_p(out.ptr), None, None) == capi.GL_ERR_INVALID_ARG
    still_works()
