"""GPU parity of the k-truss decomposition (gl_truss, SpMVPlan.truss, SpMVModule.truss, app.KTruss, graphlily::app::KTruss): every
comparison is np.array_equal against a closed form or the host peel of tests/test_truss_cpu.py, which that file checks against
networkx and a one-edge-at-a-time statement of the definition.  The result is exact and unique: no tolerance anywhere.  Output
buffers start as garbage, and every case is called twice on one plan, with and without d_support."""
import ctypes
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import named_matrix, set_knob
from test_cc_cpu import permute_rows
from test_truss_cpu import (LEVELS, RECORDS, TRUSS_DRIVER, _clique_edges, _csr, book_on_a_clique, build_cpp_driver, entry_rows,
                            glued_cliques, graph_of, prepared, summary, truss_numbers)

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _truss(plan, nnz, support=True):
    """-> (truss, support or None, stats); the buffers start out as garbage: the call writes every word itself"""
    t = capi.DeviceBuffer.from_host(np.full(nnz, GARBAGE, np.uint32))
    s = capi.DeviceBuffer.from_host(np.full(nnz, GARBAGE, np.uint32)) if support else None
    stats = plan.truss(t, s)
    capi.sync()
    assert len(stats) == 6 and 0xdeadbeefdeadbeef not in stats
    return t.read(np.uint32, nnz), (s.read(np.uint32, nnz) if support else None), stats


def _check(sym, want, want_support, sub_rounds=None, plan=None):
    """truss and support equal the closed form, the stats describe the run; with and without d_support on one plan"""
    plan = _bool_plan(sym) if plan is None else plan
    want, want_support = np.asarray(want, np.uint32), np.asarray(want_support, np.uint32)
    edges = int(np.count_nonzero(sym.adj_indices.astype(np.int64) > entry_rows(sym)))
    triangles, rest = divmod(int(want_support.astype(np.int64).sum()), 6)
    assert rest == 0
    truss, support, stats = _truss(plan, sym.nnz)
    assert np.array_equal(truss, want) and np.array_equal(support, want_support)
    assert stats[0] == int(want.max()) and stats[1] == np.unique(want[want > 0]).shape[0] and stats[4:] == (edges, triangles)
    assert 1 <= stats[2] <= edges and stats[3] >= 3 + 4
    if sub_rounds is not None:
        assert stats[2] == sub_rounds
    truss, support, again = _truss(plan, sym.nnz, support=False)       # (the second time from the cached numbering and verdicts)
    assert np.array_equal(truss, want) and support is None and again[:3] == stats[:3] and again[4:] == stats[4:]
    return stats


@pytest.mark.parametrize("k", [2, 3, 4, 17, 65, 130])
def test_cliques(gpu, k):
    """K_k on the vertices 5 .. k + 4: truss k and support k - 2 everywhere, one level, one sub-round -- every triangle has three
    edges in the slice, so nothing may be decremented.  Rows of 64 and 129 entries cross a group's and a wavefront's piece."""
    a, b = _clique_edges(k, 5)
    g = graph_of(256, a, b)
    stats = _check(g, np.full(g.nnz, k), np.full(g.nnz, k - 2), sub_rounds=1)
    assert stats[:2] == (k, 1)


@pytest.mark.parametrize("p", [1, 7, 300])
def test_book_on_a_clique(gpu, p):
    """clique edges have truss 5, pages truss 3, the spine's support is 3 + p: both pages of a triangle are in one slice and
    exactly one of them takes a triangle from the spine -- a missed or doubled tie-break shows as a spine below 5"""
    g, want, support = book_on_a_clique(p, 384)
    spine = int(g.adj_indptr[0])                                         # (row 0 starts with the entry (0, 1))
    assert g.adj_indices[spine] == 1 and support[spine] == 3 + p and want[spine] == 5
    stats = _check(g, want, support, sub_rounds=2)
    assert stats[:2] == (5, 2)


def test_wheel(gpu):
    """hub 0 and 200 rim vertices: everything has truss 3; the rim edges go first, and every spoke, at 2, receives two requests
    to come down and must stop at the level"""
    rim = np.arange(1, 201)
    g = graph_of(256, np.concatenate([np.zeros(200, np.int64), rim]), np.concatenate([rim, np.roll(rim, -1)]))
    spoke = (entry_rows(g) == 0) | (g.adj_indices == 0)
    stats = _check(g, np.full(g.nnz, 3), np.where(spoke, 2, 1), sub_rounds=2)
    assert stats[:2] == (3, 1) and stats[5] == 200


def test_bipartite_and_star_have_no_triangle(gpu):
    g = graph_of(128, np.repeat(np.arange(40), 50), np.tile(np.arange(40, 90), 40))       # K_{40,50}
    stats = _check(g, np.full(g.nnz, 2), np.zeros(g.nnz), sub_rounds=1)
    assert stats[:2] == (2, 1) and stats[4:] == (2000, 0)
    g = graph_of(5120, np.full(5000, 11), np.arange(12, 5012))          # a star with 5000 leaves
    stats = _check(g, np.full(g.nnz, 2), np.zeros(g.nnz), sub_rounds=1)
    assert stats[:2] == (2, 1) and stats[4:] == (5000, 0)


def test_hub_meets_hub(gpu):
    """0 .. 7 form K_8 and 5000 leaves are each adjacent to 0 and to 1: leaf edges have truss 3, clique edges 8, and the edge
    (0, 1) intersects two rows of 5007 entries and is asked to come down 5000 times"""
    a, b = _clique_edges(8)
    leaves = np.arange(8, 5008)
    g = graph_of(5120, np.concatenate([a, np.zeros(5000, np.int64), np.ones(5000, np.int64)]), np.concatenate([b, leaves, leaves]))
    rows, cols = entry_rows(g), g.adj_indices.astype(np.int64)
    leaf = (rows >= 8) | (cols >= 8)
    hubs = (np.minimum(rows, cols) == 0) & (np.maximum(rows, cols) == 1)
    stats = _check(g, np.where(leaf, 3, 8), np.where(leaf, 1, np.where(hubs, 5006, 6)), sub_rounds=2)
    assert stats[:2] == (8, 2) and stats[4:] == (28 + 10000, 56 + 5000)


def test_glued_cliques(gpu):
    """K_6, K_5, K_4, K_3 glued along an edge in a chain: every shared edge takes the larger truss"""
    g, want = glued_cliques(128)
    _, support, _, sub_rounds, _ = truss_numbers(g)
    stats = _check(g, want, support, sub_rounds=sub_rounds)
    assert stats[:2] == (6, 4)


def test_stored_diagonal_entries(gpu):
    """entries (v, v) get 0 in both arrays and change nothing else: the book on a clique with a diagonal entry on 0, on 1, on a page
    and on the isolated vertex 200"""
    g, want, support = book_on_a_clique(7, 256)
    rows, cols = entry_rows(g), g.adj_indices.astype(np.int64)
    diag = np.array([0, 1, 9, 200])
    r, c = np.concatenate([rows, diag]), np.concatenate([cols, diag])
    order = np.lexsort((c, r))
    d = _csr(256, r, c)
    assert np.array_equal(d.adj_indices, c[order].astype(np.uint32)) and d.nnz == g.nnz + 4
    with_zeros = lambda x: np.concatenate([x, np.zeros(4, np.uint32)])[order]
    stats = _check(d, with_zeros(want), with_zeros(support), sub_rounds=2)
    assert stats[4] == g.nnz // 2
    only = _csr(128, [3, 9], [3, 9])                                     # nothing but a diagonal: no edge
    truss, support, stats = _truss(_bool_plan(only), 2)
    assert not truss.any() and not support.any() and stats == (0, 0, 0, 0, 0, 0)


def _driver(m):
    kt = app.KTruss(M.num_hbm_channels, 1024, 256)
    kt.set_target("hw")
    kt.set_up_runtime("unused.xclbin")
    kt.load_and_format_matrix(m, True)
    kt.send_matrix_host_to_device()
    return kt


@pytest.mark.parametrize("name", ["uniform", "rmat", "rmat_sym", "messy", "many"])
def test_drivers(gpu, name):
    raw, m, sym, want, want_support, levels, sub_rounds = prepared(name)
    kt = _driver(raw)
    got = kt.run(support=True)
    assert got.dtype == np.uint32 and got.shape == (sym.nnz,) and kt.truss_ is got and kt.n_real_ == raw.num_rows
    assert np.array_equal(kt.graph_.adj_indices, sym.adj_indices) and np.array_equal(kt.graph_.adj_indptr, sym.adj_indptr)
    assert np.array_equal(got, want) and np.array_equal(kt.support_, want_support)
    assert summary(sym, got, kt.sub_rounds_, kt.num_triangles_) == RECORDS[name]         # sub_rounds_: pins the schedule
    assert (kt.max_truss_, kt.levels_, kt.num_edges_) == (RECORDS[name][0], LEVELS[name], sym.nnz // 2)
    assert kt.launches_ >= 3 + 4
    rows = entry_rows(sym)
    once = sym.adj_indices.astype(np.int64) > rows
    assert kt.truss_sizes_.shape == (kt.max_truss_ + 1,) and kt.truss_sizes_[0] == kt.truss_sizes_[2] == sym.nnz // 2
    assert all(kt.truss_sizes_[k] == np.count_nonzero(want[once] >= k) for k in range(kt.max_truss_ + 1))
    vt = np.zeros(sym.num_rows, np.uint32)
    np.maximum.at(vt, rows, want)
    assert kt.vertex_truss_.dtype == np.uint32 and np.array_equal(kt.vertex_truss_, vt) and not vt[raw.num_rows:].any()
    top = kt.k_truss(kt.max_truss_)
    assert top.dtype == bool and top.shape == (sym.nnz,) and np.array_equal(top, want == kt.max_truss_)
    assert kt.k_truss(2).all() and not kt.k_truss(kt.max_truss_ + 1).any()
    sub = kt.sub_rounds_
    assert np.array_equal(kt.run(), want) and kt.support_ is None and kt.sub_rounds_ == sub    # a second run, without the supports
    # the same graph with the entries of every row in a random order: the preparation sorts them
    assert np.array_equal(_driver(permute_rows(raw, 5)).run(), want)


def test_rmat_20K_by_its_record_and_rule_1(gpu):
    """a row of 5133 entries; the host peel takes too long here, so: no value is too high (rule 1 of validate_truss) and the sum
    over the edges is the recorded one, so no value is too low either"""
    raw = named_matrix("rmat_20K")
    kt = _driver(raw)
    got = kt.run(support=True)
    sym = kt.graph_
    assert int(np.diff(sym.adj_indptr.astype(np.int64)).max()) == 5133
    assert summary(sym, got, kt.sub_rounds_, kt.num_triangles_) == RECORDS["rmat_20K"]
    assert (kt.max_truss_, kt.levels_) == (RECORDS["rmat_20K"][0], LEVELS["rmat_20K"])
    once = sym.adj_indices.astype(np.int64) > entry_rows(sym)
    assert int(kt.support_[once].astype(np.int64).sum()) == 3 * RECORDS["rmat_20K"][2]
    assert app.validate_truss(raw, got, peel=False) == RECORDS["rmat_20K"][0]


@pytest.mark.parametrize("group", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("batch", [1, 64])
def test_knobs_change_nothing(gpu, monkeypatch, group, batch):
    """the lanes per edge and the launches between two read-backs change neither a bit of the result nor the sub-rounds, which are
    a property of the graph; the knobs are read per call"""
    _, _, sym, want, want_support, _, sub_rounds = prepared("rmat_sym")
    plan = _bool_plan(sym)
    _, _, base = _truss(plan, sym.nnz)
    book, book_want, book_support = book_on_a_clique(300, 384)
    set_knob(monkeypatch, "truss_group", group)
    set_knob(monkeypatch, "truss_batch", batch)
    truss, support, stats = _truss(plan, sym.nnz)
    assert np.array_equal(truss, want) and np.array_equal(support, want_support)
    assert stats[:3] == base[:3] and stats[4:] == base[4:] and stats[2] == sub_rounds
    assert (stats[3] - 3) % (3 * batch + 1) == 0
    _check(book, book_want, book_support, sub_rounds=2)
    set_knob(monkeypatch, "truss_grid", 1)
    truss, _, stats = _truss(plan, sym.nnz, support=False)
    assert np.array_equal(truss, want) and stats[2] == sub_rounds


@pytest.mark.parametrize("spread", [0, 7, 10, 16])
def test_lanes_given_to_short_slices_change_nothing(gpu, monkeypatch, spread):
    """a peel launch whose slice is short gives an edge up to 1 << truss_spread lanes, across wavefronts and workgroups (0: never
    more than truss_group): same bits, same sub-rounds -- on a graph whose late sub-rounds hold a few hub edges, with the lanes
    per edge starting at 4 and at the default, and on the book, whose spine has rows of 304 entries"""
    _, _, sym, want, want_support, _, sub_rounds = prepared("rmat_sym")
    book, book_want, book_support = book_on_a_clique(300, 384)
    set_knob(monkeypatch, "truss_spread", spread)
    _check(sym, want, want_support, sub_rounds=sub_rounds)
    _check(book, book_want, book_support, sub_rounds=2)
    set_knob(monkeypatch, "truss_group", 4)
    _check(sym, want, want_support, sub_rounds=sub_rounds)
    _check(book, book_want, book_support, sub_rounds=2)


@pytest.mark.parametrize("truss_first", [True, False])
def test_cross_checks_with_tc_kcore_and_color_on_one_plan(gpu, truss_first):
    """the cached verdicts in either order of first use; the triangles equal gl_tc_count's total on the oriented form; and
    truss[(u, v)] <= min(core[u], core[v]) + 1"""
    _, m, sym, want, want_support, _, sub_rounds = prepared("rmat_sym")
    n = sym.num_rows
    plan = _bool_plan(sym)
    if truss_first:
        _check(sym, want, want_support, sub_rounds=sub_rounds, plan=plan)
    core = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))
    colour = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))
    plan.kcore(core)
    plan.color(None, colour)
    capi.sync()
    core = core.read(np.uint32, n)
    assert app.validate_cores(sym, core) == int(core.max()) and app.validate_coloring(sym, colour.read(np.uint32, n), None) >= 2
    stats = _check(sym, want, want_support, sub_rounds=sub_rounds, plan=plan)
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    assert np.all(want <= np.minimum(core[rows], core[cols]) + 1)
    oriented, _ = io.triangle_orient(m)
    total = capi.DeviceBuffer(8)
    _bool_plan(oriented).tc_count(total)
    capi.sync()
    assert int(total.read(np.uint64, 1)[0]) == stats[5] == RECORDS["rmat_sym"][2]


def test_empty_plan_and_no_vertices(gpu):
    n = 256
    e = _csr(n, [], [])                          # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    out = capi.DeviceBuffer.from_host(np.full(16, GARBAGE, np.uint32))
    for _ in range(2):
        assert empty.truss(out) == (0, 0, 0, 0, 0, 0)
    capi.sync()
    assert np.all(out.read(np.uint32, 16) == GARBAGE), "a plan without entries writes nothing"
    none = capi.SpMVPlan(0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, 0, flags=capi.GL_PLAN_BOOLEAN)
    assert none.truss(out, None) == (0, 0, 0, 0, 0, 0)
    capi.sync()
    assert np.all(out.read(np.uint32, 16) == GARBAGE)
    kt = _driver(e)                                                       # the driver on a graph without edges
    assert kt.run(support=True).shape == (0,) and kt.support_.shape == (0,) and kt.max_truss_ == 0 and not kt.vertex_truss_.any()
    assert kt.truss_sizes_.tolist() == [0]


def test_refusals(gpu):
    _, _, sym, want, _, _, _ = prepared("uniform")
    n, nnz = sym.num_rows, sym.nnz
    plan = _bool_plan(sym)

    def still_works():
        truss, _, stats = _truss(plan, nnz, support=False)
        assert np.array_equal(truss, want) and stats[0] == RECORDS["uniform"][0]
    still_works()
    out = capi.DeviceBuffer.from_host(np.full(nnz + 128, GARBAGE, np.uint32))

    def refused(p, needle):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.truss(out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
            assert "gl_truss" in str(e.value)
        assert np.all(out.read(np.uint32, nnz + 128) == GARBAGE), "a refused call writes nothing"
        still_works()
    general = capi.SpMVPlan(sym.num_rows, sym.num_cols, sym.adj_indptr, sym.adj_indices, sym.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "row copy")
    refused(_bool_plan(sym, 0, n // 2), "row shard")
    refused(_bool_plan(sym, n // 2, n), "row shard")
    sh = permute_rows(sym, 77)
    assert not np.array_equal(sh.adj_indices, sym.adj_indices)
    refused(_bool_plan(sh), "io.symmetrize_simple")                        # unsorted rows
    wide = io.CSRMatrix(n, n + 128, sym.adj_data, sym.adj_indices, sym.adj_indptr)
    refused(_bool_plan(wide), "num_rows == num_cols")
    # one edge stored one way only: K_5 on 10 .. 14 in both directions, and (20, 21) without (21, 20)
    a, b = _clique_edges(5, 10)
    one_way = _csr(256, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]]))
    for needle in ("not symmetric", "io.symmetrize_simple"):
        refused(_bool_plan(one_way), needle)
    both = graph_of(256, np.concatenate([a, [20]]), np.concatenate([b, [21]]))   # with the edge's other copy it is accepted
    truss, support, stats = _truss(_bool_plan(both), both.nnz)
    assert sorted(truss.tolist()) == [2] * 2 + [5] * 20 and stats[4:] == (11, 10)
    with pytest.raises(capi.GraphLilyError) as e:
        plan.truss(None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    with pytest.raises(capi.GraphLilyError) as e:
        plan.truss(out, out)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    assert capi.lib().gl_truss(None, ctypes.c_void_p(out.ptr), None, None) == capi.GL_ERR_INVALID_ARG
    still_works()


@pytest.mark.parametrize("name", ["uniform", "rmat"])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, name):
    import scipy.sparse as sp
    build_cpp_driver("truss_driver.cpp")
    raw, m, sym, want, want_support, levels, sub_rounds = prepared(name)
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / (name + "_csr_float32.npz"))
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([TRUSS_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "KTruss::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_truss.bin"), dtype=np.uint32), want)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_support.bin"), dtype=np.uint32), want_support)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    rec = RECORDS[name]
    assert "max truss: %d\n" % rec[0] in r.stdout and "sum of truss over edges: %d\n" % rec[1] in r.stdout
    assert "triangles: %d\n" % rec[2] in r.stdout and "sub-rounds: %d\n" % rec[3] in r.stdout
    assert "checksum: %d\n" % checksum in r.stdout and "levels: %d\n" % levels in r.stdout
