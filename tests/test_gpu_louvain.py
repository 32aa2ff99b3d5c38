"""GPU parity of Louvain communities (gl_louvain_move, SpMVPlan.louvain_move, SpMVModule.louvain_move, app.Louvain,
graphlily::app::Louvain): every comparison is np.array_equal against the host move_loop() and louvain() of
tests/test_louvain_cpu.py -- labels, sweeps, moves, evaluations, stop reason, q_first and q_last per call, and the driver's
per-level arrays; that file checks the model against closed forms, networkx and app's numpy restatement, and proves that the
named inputs reach every branch of the rule.  The result is a pure function of (graph, weights, vertex weights, colouring,
max_sweeps, min_gain): no tolerance anywhere.  The output buffer starts as garbage with 64 guard words behind it and every case
is called twice on one plan."""
import ctypes
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_cc_cpu import permute_rows
from test_msf_cpu import clique_edges, raw_csr
from test_lpa_cpu import greedy_colors, lpa_case, propagate
from test_louvain_cpu import (DISCARDED_CASE, LOUVAIN_DRIVER, build_cpp_driver, driver_case, driver_graph, louvain, louvain_case, move_loop,
                              pattern_degrees, simple_graph)

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef


@pytest.fixture(autouse=True, params=[None, 0], ids=["thread_per_short_row", "wavefront_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of the rows -- a thread sums a row of at most 8 entries in registers, the
    wavefront takes the longer ones -- and with louvain_cut=0, which hands every row to the wavefront and its LDS table"""
    set_knob(monkeypatch, "louvain_cut", request.param)


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _buf(arr):
    return None if arr is None else capi.DeviceBuffer.from_host(np.ascontiguousarray(arr, np.uint32))


def _move(plan, n, weights, vweights, colors, max_sweeps, min_gain):
    """-> (labels, stats); the output buffer starts out as garbage, and a guard behind it must stay garbage"""
    out = capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32))
    stats = plan.louvain_move(out, _buf(colors), _buf(weights), _buf(vweights), max_sweeps, min_gain)
    capi.sync()
    got = out.read(np.uint32, n + 64)
    assert len(stats) == 7 and 0xdeadbeefdeadbeef not in stats and np.all(got[n:] == GARBAGE)
    return got[:n], stats


def _check(name, plan=None):
    """the labels and the stats are the host model's; twice on one plan -> the stats"""
    sym, weights, vweights, colors, max_sweeps, min_gain, want = louvain_case(name)
    plan = _bool_plan(sym) if plan is None else plan
    label, stats = _move(plan, sym.num_rows, weights, vweights, colors, max_sweeps, min_gain)
    assert np.array_equal(label, want[0])
    assert stats[:3] + stats[4:] == tuple(want[1:]), (stats, want[1:])
    assert stats[3] >= 8
    label, again = _move(plan, sym.num_rows, weights, vweights, colors, max_sweeps, min_gain)
    assert np.array_equal(label, want[0]) and again == stats
    return stats


@pytest.mark.parametrize("name", ["path_2", "path_50"])
def test_paths(gpu, name):
    want = louvain_case(name)[6]
    assert want[4] == 1 and np.array_equal(want[0][50:], np.arange(50, 128))
    _check(name)


@pytest.mark.parametrize("k", [3, 17, 65, 130])
def test_disjoint_cliques(gpu, k):
    """rows of 2, 16, 64 and 129 entries: a thread's row, the wavefront's within one step of 64, and across the 256-entry step"""
    label = louvain_case("cliques_%d" % k)[6][0]
    assert np.unique(label[5:5 + k]).shape[0] == 1
    _check("cliques_%d" % k)


@pytest.mark.parametrize("leaves", [255, 256, 257])
def test_rows_at_the_edges_of_a_wavefront_step(gpu, leaves):
    """a hub of 255, 256 and 257 entries: one step short by one, one full step, one step and one entry"""
    _check("row_%d" % leaves)


@pytest.mark.parametrize("table", [None, 8, 32])
@pytest.mark.parametrize("name", ["star_3000", "hubs"])
def test_hubs_meet_more_labels_than_the_table_holds(gpu, monkeypatch, name, table):
    """a star of 3000 leaves whose hub is colour 0, and two hubs sharing 300 leaves: in sweep 1 a hub meets 3000 (300) distinct
    labels -- more than the default table of 2048 slots holds, and far more than 8 or 32: the row is summed partition by partition"""
    set_knob(monkeypatch, "louvain_table", table)
    _check(name)


def test_every_branch_of_the_rule(gpu, monkeypatch):
    """a tie towards the smaller label, a move whose best score is negative, a stay on best == cur, weights above 1 and internal
    weight: after one sweep, after two, and at the end (tests/test_louvain_cpu.py proves that the input reaches them)"""
    sym, weights, vweights, colors, _, _, want = louvain_case("branches")
    plan = _bool_plan(sym)
    _check("branches", plan=plan)
    for sweeps in (1, 2):
        label, stats = _move(plan, sym.num_rows, weights, vweights, colors, sweeps, 0)
        model = move_loop(sym, weights, vweights, colors, sweeps, 0)
        assert np.array_equal(label, model[0]) and stats[:3] + stats[4:] == tuple(model[1:])
    assert (label[10], label[20], label[30], label[40]) == (11, 22, 30, 41)
    set_knob(monkeypatch, "louvain_table", 8)
    _check("branches", plan=plan)


@pytest.mark.parametrize("name", ["planted", "planted_weighted", "rmat", "rmat_weighted", "q_falls"])
def test_planted_partition_and_rmat(gpu, name):
    """20 blocks of 60 vertices and a small R-MAT under largest-first colourings, with unit weights and with random integer
    weights 1 .. 1000 and random internal weights; and the small G(n, p) whose last sweep loses (stop reason 2)"""
    want = louvain_case(name)[6]
    assert want[1] >= 2 and want[2] > 0 and want[6] > want[5]
    _check(name)


def test_max_sweeps_one_below_the_converging_count(gpu):
    full, short = louvain_case("planted_weighted")[6], louvain_case("planted_short")[6]
    assert short[1] == full[1] - 1 and short[4] == 0
    assert _check("planted_short")[4] == 0


def test_min_gain_large_enough_to_stop_after_sweep_one(gpu):
    want = louvain_case("planted_gain")[6]
    assert want[1] == 1 and want[4] == 2 and want[2] > 0
    assert _check("planted_gain")[:1] + _check("planted_gain")[4:5] == (1, 2)


@pytest.mark.parametrize("knob,values", [("louvain_batch", (1, 64)), ("louvain_grid", (1, 7)), ("louvain_cut", (0,)), ("louvain_table", (8,))])
def test_schedule_independence(gpu, monkeypatch, knob, values):
    """the sweeps between two read-backs, the grid, the cut and the table change no bit of the result or of the statistics"""
    plan = _bool_plan(louvain_case("planted_weighted")[0])
    base = _check("planted_weighted", plan=plan)
    for value in values:
        set_knob(monkeypatch, knob, value)
        got = _check("planted_weighted", plan=plan)
        assert got[:3] + got[4:] == base[:3] + base[4:]
        for name in ("cliques_130", "hubs", "rmat_weighted", "row_257"):
            _check(name)
    set_knob(monkeypatch, "louvain_batch", 1)                             # and batch 1 together with the knob's last setting
    _check("planted_weighted", plan=plan)


def test_no_edges(gpu):
    n = 256
    e = raw_csr(n, [], [], [])                   # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        label, stats = _move(empty, n, None, None, np.zeros(n, np.uint32), 5, 0)
        assert np.array_equal(label, np.arange(n)) and stats[:3] == (1, 0, 0) and stats[3] >= 1 and stats[4:] == (1, 0, 0)
    only = raw_csr(128, [3, 9], [3, 9], [1.0, 1.0])                      # nothing but a diagonal: nobody has a neighbour
    label, stats = _move(_bool_plan(only), 128, None, None, np.zeros(128, np.uint32), 5, 0)
    assert np.array_equal(label, np.arange(128)) and stats[:3] == (1, 0, 0) and stats[4:] == (1, 0, 0)


def test_refusals(gpu):
    sym, weights, vweights, colors, max_sweeps, min_gain, want = louvain_case("planted_weighted")
    n = sym.num_rows
    plan = _bool_plan(sym)

    def still_works():
        assert np.array_equal(_move(plan, n, weights, vweights, colors, max_sweeps, min_gain)[0], want[0])
    still_works()
    out = capi.DeviceBuffer.from_host(np.full(n + 128, GARBAGE, np.uint32))
    col = _buf(np.concatenate([colors, np.zeros(128, np.uint32)]))

    def refused(p, needle):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.louvain_move(out, col, None, None, 10, 0)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
            assert "gl_louvain_move" in str(e.value)
        assert np.all(out.read(np.uint32, n + 128) == GARBAGE), "a refused call writes nothing"
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
    a, b = clique_edges(5, 10)                                              # one edge stored one way only
    one_way = raw_csr(n, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]]), np.ones(21))
    for needle in ("not symmetric", "io.symmetrize_simple"):
        refused(_bool_plan(one_way), needle)

    def invalid(needle, colors_=colors, weights_=weights, vweights_=vweights, sweeps=10, label=out, code=capi.GL_ERR_INVALID_ARG, p=plan):
        for _ in range(2):
            with pytest.raises(capi.GraphLilyError) as e:
                p.louvain_move(label, _buf(colors_), _buf(weights_), _buf(vweights_), sweeps, 0)
            assert e.value.code == code and needle in str(e.value) and "gl_louvain_move" in str(e.value), str(e.value)
        assert np.all(out.read(np.uint32, n + 128)[n:] == GARBAGE)
        still_works()
    invalid("d_label", label=None)
    invalid("d_color", colors_=None)
    invalid("max_sweeps", sweeps=0)
    assert np.all(out.read(np.uint32, n + 128) == GARBAGE)
    with pytest.raises(capi.GraphLilyError) as e:                           # d_color == d_label
        plan.louvain_move(col, col, None, None, 10, 0)
    assert e.value.code == capi.GL_ERR_INVALID_ARG and "d_color != d_label" in str(e.value)
    bad = colors.copy()
    bad[5] = n
    invalid("1 words of d_color hold a colour >= n", colors_=bad)
    u = int(sym.adj_indices[sym.adj_indptr[0]])                             # vertex 0 gets its first neighbour's colour
    bad = colors.copy()
    bad[0] = colors[u]
    row = sym.adj_indices[sym.adj_indptr[0]:sym.adj_indptr[1]].astype(np.int64)
    invalid("not a proper colouring: %d entries" % (2 * int(np.count_nonzero(colors[row] == colors[u]))), colors_=bad)
    bad = weights.copy()
    bad[[3, 700]] = 0
    invalid("2 words of d_weight are zero", weights_=bad)
    bad = vweights.copy()
    first = int(np.flatnonzero(np.diff(sym.adj_indptr.astype(np.int64)))[0])
    bad[first] = int(weights[sym.adj_indptr[first]:sym.adj_indptr[first + 1]].astype(np.int64).sum()) - 1
    invalid("1 words of d_vertex_weight are below the sum", vweights_=bad)
    pair = simple_graph(128, [0], [1])                                      # two vertices of weight 2^30: two_m = 2^31
    heavy = np.zeros(128, np.uint32)
    heavy[:2] = 1 << 30
    two = np.zeros(128, np.uint32)
    two[1] = 1
    pair_plan = _bool_plan(pair)
    invalid("two_m = 2147483648 >= 2^31", colors_=two, weights_=None, vweights_=heavy, code=capi.GL_ERR_UNSUPPORTED, p=pair_plan)
    heavy[1] -= 1                                                           # ... and one below the bound runs: the score 2^31 - 1 - 2^30 (2^30 - 1) is negative, both stay
    label, stats = _move(pair_plan, 128, None, heavy, two, 10, 0)
    model = move_loop(pair, None, heavy, two, 10, 0)
    assert np.array_equal(label, model[0]) and stats[:3] + stats[4:] == tuple(model[1:]) and (label[0], label[1], model[2]) == (0, 1, 0)
    assert capi.lib().gl_louvain_move(None, None, None, ctypes.c_void_p(col.ptr), ctypes.c_void_p(out.ptr), 1, 0, None) == capi.GL_ERR_INVALID_ARG
    still_works()


def test_label_propagation_on_the_same_plan_is_untouched(gpu):
    """gl_lpa before and after a gl_louvain_move call on one plan gives the same bits: the two scratch areas are separate"""
    sym, colors, init, max_sweeps, want = lpa_case("planted")
    n = sym.num_rows
    plan = _bool_plan(sym)

    def lpa():
        out = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))
        stats = plan.lpa(out, _buf(colors), _buf(init), max_sweeps)
        capi.sync()
        return out.read(np.uint32, n), stats[:3] + stats[4:]
    before = lpa()
    assert np.array_equal(before[0], want[0])
    label, stats = _move(plan, n, None, None, colors, 100, 0)
    model = louvain_case("planted")[6]
    assert np.array_equal(label, model[0]) and stats[:3] + stats[4:] == tuple(model[1:])
    after = lpa()
    assert np.array_equal(after[0], before[0]) and after[1] == before[1]
    assert np.array_equal(_move(plan, n, None, None, colors, 100, 0)[0], model[0])


def _driver(m):
    d = app.Louvain(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True)
    d.send_matrix_host_to_device()
    return d


def _same_as_model(d, got, want):
    assert np.array_equal(got, want["labels"]) and d.levels_ == want["levels"]
    assert np.array_equal(d.level_sizes_, want["sizes"]) and np.array_equal(d.level_colors_, want["colors"])
    assert np.array_equal(d.level_sweeps_, want["sweeps"]) and np.array_equal(d.level_moves_, want["moves"])
    assert d.level_q_.dtype == np.int64 and np.array_equal(d.level_q_, np.asarray(want["q"], dtype=np.int64).reshape(-1, 2))
    assert len(d.dendrogram_) == want["levels"] and all(np.array_equal(a, b) for a, b in zip(d.dendrogram_, want["dendrogram"]))


@pytest.mark.parametrize("order", io.COLORING_ORDERS)
@pytest.mark.parametrize("name", ["planted", "rmat"])
def test_driver_with_every_order(gpu, name, order):
    raw, sym = driver_graph(name)
    d = _driver(raw)
    got = d.run(order=order)
    n = sym.num_rows
    assert got.dtype == np.uint32 and got.shape == (n,) and d.labels_ is got and d.n_real_ == raw.num_rows
    if order != "smallest_last":                                           # (the peeling order is not unique)
        assert np.array_equal(d.level_colorings_[0], greedy_colors(sym, io.coloring_priorities(pattern_degrees(sym), order, 0)))
        want = driver_case(name, order)
    else:
        want = louvain(sym, colorings=d.level_colorings_)
    _same_as_model(d, got, want)
    assert app.validate_louvain(raw, got, order=order, colorings=d.level_colorings_) == np.unique(got).shape[0]
    labels, sizes = np.unique(got[:d.n_real_], return_counts=True)
    assert d.num_communities_ == labels.shape[0] and np.array_equal(d.community_labels_, labels) and np.array_equal(d.community_sizes_, sizes)
    two_m = float(sym.nnz)
    accepted = d.level_q_[d.levels_ - 1, 1] if d.levels_ else d.level_q_[0, 0]
    assert abs(d.modularity() - accepted / two_m ** 2) < 1e-12 and d.modularity() == d.modularity(got) and d.launches_ >= 8
    lpa = propagate(sym, d.level_colorings_[0], None, 100)[0]
    assert d.modularity() >= d.modularity(lpa)
    # a second run ("smallest_last" may peel in another order: only the shape of the result is the same)
    again = d.run(order=order)
    assert np.array_equal(again, got) if order != "smallest_last" else again.shape == got.shape


def test_driver_discards_a_level_that_loses(gpu):
    name, order = DISCARDED_CASE
    raw, sym = driver_graph(name)
    want = driver_case(name, order)
    assert want["discarded"]
    d = _driver(raw)
    _same_as_model(d, d.run(order=order), want)
    assert len(d.level_sizes_) == d.levels_ + 1 and d.level_moves_[-1] > 0 and d.level_q_[-1, 1] <= d.level_q_[-1, 0]
    got = d.run(order=order, max_levels=1)
    _same_as_model(d, got, louvain(sym, order=order, max_levels=1))
    got = d.run(order=order, max_sweeps=1, tol=0.0)
    _same_as_model(d, got, louvain(sym, order=order, max_sweeps=1, tol=0.0))


@pytest.mark.parametrize("name,order,seed", [("planted", "largest_first", 0), ("rmat", "largest_first", 0), ("rmat", "random", 3), ("planted", "natural", 0)])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, name, order, seed):
    import scipy.sparse as sp
    build_cpp_driver("louvain_driver.cpp")
    raw, sym = driver_graph(name)
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / "graph_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([LOUVAIN_DRIVER, path, str(tmp_path), order, str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Louvain::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(raw)
    want = d.run(order=order, seed=seed)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_label.bin"), dtype=np.uint32), want)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    lines = ["levels: %d" % d.levels_, "launches: %d" % d.launches_, "communities: %d" % d.num_communities_, "checksum: %d" % checksum]
    lines += ["level %d: size %d colours %d sweeps %d moves %d q_first %d q_last %d" % (i, d.level_sizes_[i], d.level_colors_[i], d.level_sweeps_[i],
                                                                                     d.level_moves_[i], d.level_q_[i, 0], d.level_q_[i, 1])
              for i in range(len(d.level_sizes_))]
    for line in lines:
        assert line + "\n" in r.stdout, (line, r.stdout[-1500:])
    q = float([l for l in r.stdout.splitlines() if l.startswith("modularity: ")][0].split()[1])
    assert abs(q - d.modularity()) < 1e-9
