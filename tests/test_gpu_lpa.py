"""GPU parity of label propagation communities (gl_lpa, SpMVPlan.lpa, SpMVModule.lpa, app.LabelPropagation,
graphlily::app::LabelPropagation): every comparison is np.array_equal against the host propagate() of tests/test_lpa_cpu.py, and
sweeps, changes, evaluations and converged equal its counts; that file checks it against closed forms, both invariants and
app._lpa_color_loop.  The result is a pure function of (graph, colouring, initial labels): no tolerance anywhere.  The output
buffer starts as garbage with 64 guard words behind it and every case is called twice on one plan."""
import ctypes
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import named_matrix, set_knob
from test_cc_cpu import permute_rows
from test_msf_cpu import clique_edges, raw_csr
from test_lpa_cpu import (COLOR_CASES, LPA_DRIVER, SYNC_CASES, TOP, branches_graph, build_cpp_driver, greedy_colors, largest_first,
                          lpa_case, propagate)

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef


@pytest.fixture(autouse=True, params=[None, 0], ids=["thread_per_short_row", "wavefront_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of the rows -- a thread counts a row of at most 8 entries in registers,
    the wavefront takes the longer ones -- and with lpa_cut=0, which hands every row to the wavefront and its LDS table"""
    set_knob(monkeypatch, "lpa_cut", request.param)


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _buf(arr):
    return None if arr is None else capi.DeviceBuffer.from_host(np.ascontiguousarray(arr, np.uint32))


def _lpa(plan, n, colors, init, max_sweeps):
    """-> (labels, stats); the output buffer starts out as garbage, and a guard behind it must stay garbage"""
    out = capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32))
    stats = plan.lpa(out, _buf(colors), _buf(init), max_sweeps)
    capi.sync()
    got = out.read(np.uint32, n + 64)
    assert len(stats) == 5 and 0xdeadbeefdeadbeef not in stats and np.all(got[n:] == GARBAGE)
    return got[:n], stats


def _check(name, plan=None, evaluations=None):
    """the labels and the stats are the host model's; twice on one plan -> the stats"""
    sym, colors, init, max_sweeps, want = lpa_case(name)
    plan = _bool_plan(sym) if plan is None else plan
    label, stats = _lpa(plan, sym.num_rows, colors, init, max_sweeps)
    assert np.array_equal(label, want[0])
    assert (stats[0], stats[1], stats[4]) == (want[1], want[2], want[4]), (stats, want[1:])
    assert stats[2] == (want[3] if evaluations is None else evaluations) and stats[3] >= 2
    label, again = _lpa(plan, sym.num_rows, colors, init, max_sweeps)
    assert np.array_equal(label, want[0]) and again == stats
    return stats


@pytest.mark.parametrize("name", ["path_2", "path_natural"])
def test_paths(gpu, name):
    """600 used vertices of 640: a path under a 2-colouring, and the path through a shuffled vertex order under the colouring a
    greedy pass in natural order gives; the 40 unused vertices keep their numbers"""
    sym, colors, _, _, want = lpa_case(name)
    assert int(colors.max()) + 1 == (2 if name == "path_2" else 3) and want[4] == 1
    _check(name)
    assert np.array_equal(want[0][600:], np.arange(600, 640))


@pytest.mark.parametrize("k", [3, 17, 65, 130])
def test_disjoint_cliques(gpu, k):
    """rows of 2, 16, 64 and 129 entries: a thread's row, the wavefront's within one step of 64, and across the 256-entry step"""
    label = lpa_case("cliques_%d" % k)[4][0]
    assert np.unique(label[5:5 + k]).tolist() == [6]
    assert _check("cliques_%d" % k)[0] == 2


@pytest.mark.parametrize("table", [None, 8, 32])
@pytest.mark.parametrize("name", ["star", "hubs"])
def test_hubs_meet_more_labels_than_the_table_holds(gpu, monkeypatch, name, table):
    """a star with 600 leaves, and two hubs sharing 300 leaves: in sweep 1 a hub meets 600 (300) distinct labels.  At the default
    table they fit; with lpa_table below 64 slots the row is counted partition by partition"""
    set_knob(monkeypatch, "lpa_table", table)
    _check(name)


@pytest.mark.parametrize("name", ["branches_1", "branches"])
def test_every_branch_of_the_rule(gpu, monkeypatch, name):
    """a tie that excludes the current label takes the smallest, one that includes it keeps it, a strict gain moves the vertex,
    cur = 0, initial labels that are not injective, labels up to 0xfffffffe -- after one sweep, and at the fixed point"""
    sym, colors, init, after = branches_graph()
    plan = _bool_plan(sym)
    _check(name, plan=plan)
    label, _ = _lpa(plan, sym.num_rows, colors, init, 1)
    assert {c: int(label[c]) for c in after} == after and int(label.max()) == TOP
    set_knob(monkeypatch, "lpa_table", 8)
    _check(name, plan=plan)


@pytest.mark.parametrize("name", ["planted", "planted_seeded", "rmat"])
def test_planted_partition_and_rmat(gpu, name):
    """20 blocks of 60 vertices (p_in 0.3, p_out 0.005) and rmat_20K symmetrised, under largest-first colourings: ties everywhere,
    many classes, an active set that shrinks"""
    sym, colors, init, _, want = lpa_case(name)
    linked = int(np.count_nonzero(np.diff(sym.adj_indptr.astype(np.int64))))
    assert want[4] == 1 and want[1] >= 3 and linked < want[3] < linked * want[1] and int(colors.max()) >= 9
    _check(name)


@pytest.mark.parametrize("name", SYNC_CASES)
def test_synchronous_schedule(gpu, name):
    """K_{5,7} and a path flip for ever: 6 and 7 sweeps end in either of the two buffers, converged == 0; a clique converges"""
    want = lpa_case(name)[4]
    assert want[4] == (1 if name == "sync_clique_100" else 0)
    _check(name)


def test_max_sweeps_one_below_the_converging_count(gpu):
    """the labels are final already, and the run does not know it: converged == 0"""
    full, short = lpa_case("planted"), lpa_case("planted_short")
    assert short[3] == full[4][1] - 1 and short[4][4] == 0 and np.array_equal(short[4][0], full[4][0])
    assert _check("planted_short")[4] == 0


@pytest.mark.parametrize("knob,values", [("lpa_batch", (1, 64)), ("lpa_cut", (0,)), ("lpa_grid", (1, 7)), ("lpa_table", (8,)), ("lpa_active", (0, 1))])
def test_schedule_independence(gpu, monkeypatch, knob, values):
    """the sweeps between two read-backs, the cut, the grid, the table and the active set change neither a bit of the result nor
    sweeps, changes and converged; with lpa_active=0 evaluations is vertices with a neighbour x sweeps.  The knobs are read per call"""
    sym, colors, init, max_sweeps, want = lpa_case("planted")
    plan = _bool_plan(sym)
    base = _check("planted", plan=plan)
    linked = int(np.count_nonzero(np.diff(sym.adj_indptr.astype(np.int64))))
    for value in values:
        set_knob(monkeypatch, knob, value)
        every = (knob, value) == ("lpa_active", 0)
        got = _check("planted", plan=plan, evaluations=linked * want[1] if every else None)
        assert (got[0], got[1], got[4]) == (base[0], base[1], base[4])
        for name in ("cliques_130", "hubs", "path_natural", "sync_path_7"):
            s, w = lpa_case(name)[0], lpa_case(name)[4]
            _check(name, evaluations=int(np.count_nonzero(np.diff(s.adj_indptr.astype(np.int64)))) * w[1] if every else None)
    set_knob(monkeypatch, "lpa_batch", 1)                                 # and batch 1 together with the knob's last setting
    every = knob == "lpa_active" and values[-1] == 0
    _check("planted", plan=plan, evaluations=linked * want[1] if every else None)


def test_no_edges(gpu):
    n = 256
    e = raw_csr(n, [], [], [])                   # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    init = np.arange(n, dtype=np.uint32)[::-1] * 3
    for _ in range(2):
        label, stats = _lpa(empty, n, None, None, 5)
        assert np.array_equal(label, np.arange(n)) and stats[:3] == (1, 0, 0) and stats[3] >= 1 and stats[4] == 1
        label, stats = _lpa(empty, n, np.zeros(n, np.uint32), init, 5)
        assert np.array_equal(label, init) and stats[:3] == (1, 0, 0) and stats[4] == 1
    only = raw_csr(128, [3, 9], [3, 9], [1.0, 1.0])                      # nothing but a diagonal: nobody has a neighbour
    label, stats = _lpa(_bool_plan(only), 128, np.zeros(128, np.uint32), None, 5)
    assert np.array_equal(label, np.arange(128)) and (stats[0], stats[1], stats[2], stats[4]) == (1, 0, 0, 1)


def test_refusals(gpu):
    sym, colors, init, max_sweeps, want = lpa_case("planted")
    n = sym.num_rows
    plan = _bool_plan(sym)

    def still_works():
        assert np.array_equal(_lpa(plan, n, colors, init, max_sweeps)[0], want[0])
    still_works()
    out = capi.DeviceBuffer.from_host(np.full(n + 128, GARBAGE, np.uint32))
    col = _buf(np.concatenate([colors, np.zeros(128, np.uint32)]))

    def refused(p, needle):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.lpa(out, col, None, 10)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
            assert "gl_lpa" in str(e.value)
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

    def invalid(needle, colors_=colors, init_=init, sweeps=10, label=out):
        for _ in range(2):
            with pytest.raises(capi.GraphLilyError) as e:
                plan.lpa(label, _buf(colors_), _buf(init_), sweeps)
            assert e.value.code == capi.GL_ERR_INVALID_ARG and needle in str(e.value) and "gl_lpa" in str(e.value), str(e.value)
        assert np.all(out.read(np.uint32, n + 128)[n:] == GARBAGE)
        still_works()
    invalid("d_label", label=None)
    invalid("max_sweeps", sweeps=0)
    assert np.all(out.read(np.uint32, n + 128) == GARBAGE)
    bad = np.arange(n, dtype=np.uint32)
    bad[17] = bad[900] = 0xffffffff
    invalid("2 words of d_init hold the label 0xffffffff", init_=bad)
    bad = colors.copy()
    bad[5] = n
    invalid("1 words of d_color hold a colour >= n", colors_=bad)
    u = int(sym.adj_indices[sym.adj_indptr[0]])                             # vertex 0 gets its first neighbour's colour
    bad = colors.copy()
    bad[0] = colors[u]
    row = sym.adj_indices[sym.adj_indptr[0]:sym.adj_indptr[1]].astype(np.int64)
    invalid("not a proper colouring: %d entries" % (2 * int(np.count_nonzero(colors[row] == colors[u]))), colors_=bad)
    assert capi.lib().gl_lpa(None, None, None, ctypes.c_void_p(out.ptr), 1, None) == capi.GL_ERR_INVALID_ARG
    still_works()


def _driver(m):
    d = app.LabelPropagation(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True)
    d.send_matrix_host_to_device()
    return d


def _driver_graph():
    raw = named_matrix("uniform_10K_10")
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    return raw, m, io.symmetrize_simple(m)[0]


@pytest.mark.parametrize("order", io.COLORING_ORDERS)
def test_driver_with_every_order(gpu, order):
    raw, m, sym = _driver_graph()
    d = _driver(raw)
    got = d.run(order=order)
    n = sym.num_rows
    assert got.dtype == np.uint32 and got.shape == (n,) and d.labels_ is got and d.n_real_ == raw.num_rows and d.initial_ is None
    assert d.colors_.shape == (n,) and int(d.colors_.max()) + 1 == d.num_colors_
    if order != "smallest_last":                                           # (the peeling order is not unique)
        deg = np.diff(sym.adj_indptr.astype(np.int64)).astype(np.uint32)
        assert np.array_equal(d.colors_, greedy_colors(sym, io.coloring_priorities(deg, order, 0)))
    want = propagate(sym, d.colors_, None, 100)
    assert np.array_equal(got, want[0])
    assert (d.sweeps_, d.changes_, d.evaluations_, d.converged_) == want[1:] and d.converged_ == 1 and d.launches_ >= 2
    assert app.validate_communities(m, got, d.colors_) == np.unique(got).shape[0]
    labels, sizes = np.unique(got[:d.n_real_], return_counts=True)
    assert d.num_communities_ == labels.shape[0] and np.array_equal(d.community_labels_, labels) and np.array_equal(d.community_sizes_, sizes)
    assert np.array_equal(got[d.n_real_:], np.arange(d.n_real_, n))
    assert -0.5 <= d.modularity() <= 1.0 and d.modularity() == d.modularity(got)
    # a second run (gl_kcore's peeling order is not unique, so "smallest_last" repeats under the first run's colouring)
    assert np.array_equal(d.run(order=order) if order != "smallest_last" else d.run(colors=d.colors_), got)


def test_driver_with_seed_colors_initial_and_synchronous(gpu):
    raw, m, sym = _driver_graph()
    n = sym.num_rows
    d = _driver(raw)
    got = d.run(seed=5)
    start = io.lpa_initial_labels(raw.num_rows, 5, n)
    assert np.array_equal(d.initial_, start)
    deg = np.diff(sym.adj_indptr.astype(np.int64)).astype(np.uint32)
    assert np.array_equal(d.colors_, greedy_colors(sym, io.coloring_priorities(deg, "largest_first", 5)))
    want = propagate(sym, d.colors_, start, 100)
    assert np.array_equal(got, want[0]) and (d.sweeps_, d.changes_, d.evaluations_, d.converged_) == want[1:]
    assert app.validate_communities(m, got, d.colors_, start) == np.unique(got).shape[0]
    colors = greedy_colors(sym)                                            # the caller's colouring, and the caller's labels
    mine = (np.arange(raw.num_rows, dtype=np.uint32) // 7) * 7 + 3
    got = d.run(colors=colors[:raw.num_rows], initial=mine, max_sweeps=3)
    full = np.concatenate([mine, np.arange(raw.num_rows, n, dtype=np.uint32)])
    want = propagate(sym, colors, full, 3)
    assert np.array_equal(got, want[0]) and (d.sweeps_, d.changes_, d.evaluations_, d.converged_) == want[1:]
    assert app.validate_communities(m, got, colors, full, 3) > 0 and np.array_equal(d.colors_, colors)
    got = d.run(synchronous=True, max_sweeps=5)
    want = propagate(sym, None, None, 5, True)
    assert np.array_equal(got, want[0]) and (d.sweeps_, d.changes_, d.evaluations_, d.converged_) == want[1:] and d.colors_ is None
    assert app.validate_communities(m, got, None, None, 5) > 0
    with pytest.raises(ValueError, match="initial of shape"):
        d.run(initial=np.arange(5))
    with pytest.raises(ValueError, match="colors of shape"):
        d.run(colors=np.arange(5))
    with pytest.raises(capi.GraphLilyError, match="not a proper colouring"):
        d.run(colors=np.zeros(n, np.uint32))


@pytest.mark.parametrize("order,seed,sweeps,sync", [("largest_first", -1, 100, 0), ("natural", 4, 100, 0), ("random", -1, 2, 0), ("largest_first", -1, 5, 1)])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, order, seed, sweeps, sync):
    import scipy.sparse as sp
    build_cpp_driver("lpa_driver.cpp")
    raw = named_matrix("uniform_10K_10")
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / "uniform_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([LPA_DRIVER, path, str(tmp_path), order, str(seed), str(sweeps), str(sync)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LabelPropagation::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(raw)
    want = d.run(max_sweeps=sweeps, seed=None if seed < 0 else seed, order=order, synchronous=bool(sync))
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_label.bin"), dtype=np.uint32), want)
    colors = np.fromfile(str(tmp_path / "cpp_color.bin"), dtype=np.uint32)
    assert colors.shape == (0,) if sync else np.array_equal(colors, d.colors_)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    for line in ("sweeps: %d" % d.sweeps_, "changes: %d" % d.changes_, "evaluations: %d" % d.evaluations_, "converged: %d" % d.converged_,
                 "colours: %d" % d.num_colors_, "communities: %d" % d.num_communities_, "checksum: %d" % checksum):
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])
    q = float([l for l in r.stdout.splitlines() if l.startswith("modularity: ")][0].split()[1])
    assert abs(q - d.modularity()) < 1e-9
