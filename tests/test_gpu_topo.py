"""GPU parity of the topological levels and critical paths (gl_topo, SpMVPlan.topo, SpMVModule.topo, app.TopologicalOrder,
graphlily::app::TopologicalOrder) against the host model kept in tests/test_topo_cpu.py (topo_model, which that file checks against
networkx and the closed forms).  level, dist, parent and the first three stats are functions of (graph, weights), so every
comparison is exact, dist as 32-bit words.  Every test runs with the default dealing of the rows and with topo_cut=0, every output
buffer starts as garbage with 64 guard words behind it, the weights are read only, and every case is called twice on one pair of
plans.  This kernel's walk, contract and batch tests live here; the shared suites are a follow-up."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_cc_cpu import permute_rows
from test_kcore_cpu import _csr
from test_scc_cpu import scc_case
from test_topo_cpu import (ACYCLIC, CASES, GOLDEN, NAN_BITS, NONE, TOPO_DRIVER, WEIGHTS, bits, build_cpp_driver, topo_case, topo_expected,
                           topo_model, topo_weights, transposed_weights)

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef
PLAIN = WEIGHTS[:7]                     # every case; the peak / tie sets go to the cases whose rows are long
LONG_ROWS = ("fan_lengths", "fan_lengths_perm", "tournament_70", "tournament_70_perm", "in_hub_1000", "in_hub_1000_perm")


@pytest.fixture(autouse=True, params=[None, 0], ids=["thread_per_short_row", "wavefront_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of the rows -- a thread reads the first topo_cut entries of its rows, the
    wavefront takes over what is left -- and with topo_cut=0, which hands every row to the wavefront"""
    set_knob(monkeypatch, "topo_cut", request.param)


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean" or m.nnz == 0
    return plan


def _plans(cin, cout):
    return _bool_plan(cin), (None if cout is None else _bool_plan(cout))


def _topo(pin, pout, n, w=None, want_order=True):
    """-> (level, order, dist bits, parent, stats); every output starts out as garbage, and a guard behind each must stay garbage"""
    fresh = lambda: capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32))
    level, order = fresh(), fresh() if want_order else None
    dw = dist = parent = None
    if w is not None:
        dw, dist, parent = capi.DeviceBuffer.from_host(np.ascontiguousarray(w, np.float32)), fresh(), fresh()
    stats = pin.topo(pout, level, order, dw, dist, parent)
    capi.sync()
    got = []
    for buf in (level, order, dist, parent):
        if buf is None:
            got.append(None)
            continue
        words = buf.read(np.uint32, n + 64)
        assert np.all(words[n:] == GARBAGE), "a guard word was written"
        got.append(words[:n])
    assert len(stats) == 4 and 0xdeadbeefdeadbeef not in stats
    if w is not None and len(w):
        assert np.array_equal(bits(dw.read(np.float32, len(w))), bits(w)), "the weights are read only"
    return got[0], got[1], got[2], got[3], stats


def _compare(got, want, n):
    level, order, dist, parent, stats = got
    wl, wd, wp, wstats = want
    assert np.array_equal(level, wl), "level: first difference at vertex %d" % int(np.flatnonzero(level != wl)[0])
    assert stats[:3] == wstats and stats[3] >= 1
    if wd is not None:
        assert np.array_equal(dist, bits(wd)), "dist: first difference at vertex %d" % int(np.flatnonzero(dist != bits(wd))[0])
        assert np.array_equal(parent, wp), "parent: first difference at vertex %d" % int(np.flatnonzero(parent != wp)[0])
    if order is not None:
        peeled = stats[0]
        head = order[:peeled].astype(np.int64)
        assert np.array_equal(np.sort(head), np.flatnonzero(wl != NONE)), "order is no permutation of the peeled vertices"
        assert np.all(np.diff(wl[head].astype(np.int64)) >= 0), "order is not grouped by level"
        assert np.all(order[peeled:] == NONE)


def _check(name, kind=None, plans=None, reverse=False, calls=2):
    """level, dist, parent and {peeled, levels, widest} are the model's; twice on one pair of plans"""
    cin, cout, _, _ = topo_case(name)
    n = cin.num_rows
    pin, pout = _plans(cin, cout) if plans is None else plans
    w = None if kind is None else topo_weights(name, kind)
    if reverse:
        w = None if w is None else transposed_weights(name, w)
        if pout is not None:
            pin, pout = pout, pin
    want = topo_expected(name, kind, reverse)
    for _ in range(calls):                                            # (the second time from the cached verdicts and scratch)
        got = _topo(pin, pout, n, w)
        _compare(got, want, n)
    return got


@pytest.mark.parametrize("name", CASES)
def test_every_named_case(gpu, name):
    plans = _plans(*topo_case(name)[:2])
    _check(name, None, plans)
    for kind in PLAIN + (WEIGHTS[7:] if name in LONG_ROWS else ()):
        _check(name, kind, plans)
    got = _topo(*plans, topo_case(name)[0].num_rows, None, want_order=False)        # d_order may be NULL
    assert np.array_equal(got[0], topo_expected(name)[0]) and got[4][:3] == topo_expected(name)[3]


def _path(k, n):
    s = np.arange(k - 1)
    cin, cout, _ = io.simple_pattern(_csr(n, s + 1, s))
    return cin, cout, s, s + 1


@pytest.mark.parametrize("name", ["path_600", "grid_24x24_perm", "tree_1023", "in_hub_1000", "tournament_70", "lollipop", "random_1000_1400"])
def test_results_do_not_depend_on_the_batch(gpu, monkeypatch, name):
    """path_600, tree_1023, in_hub_1000 and tournament_70 have an even number of levels: under topo_batch=2 their last level ends
    exactly on a batch edge; grid_24x24 has 47: one step past it"""
    plans = _plans(*topo_case(name)[:2])
    for batch in (None, 1, 2):
        set_knob(monkeypatch, "topo_batch", batch)
        _check(name, None, plans, calls=1)
        _check(name, "signed", plans, calls=1)
    set_knob(monkeypatch, "topo_batch", 7)
    set_knob(monkeypatch, "topo_grid", 1)
    _check(name, "fractions", plans, calls=1)


@pytest.mark.parametrize("k", [63, 64, 65, 128, 129])
def test_default_batch_edges(gpu, k):
    """a path of k vertices next to 160 - k isolated ones is k levels: with the default topo_batch = 64 the runs of 64 and 128 levels
    end exactly on a batch edge, those of 65 and 129 one step past it"""
    cin, cout, src, dst = _path(k, 160)
    w = (np.arange(k - 1) % 5 - 1).astype(np.float32)
    want = topo_model(160, src, dst, w)
    assert want[3] == (160, k, 160 - k + 1)
    pin, pout = _plans(cin, cout)
    for _ in range(2):
        _compare(_topo(pin, pout, 160, w), want, 160)


@pytest.mark.parametrize("name", [c for c in CASES if c not in ("symmetric", "empty")])
def test_swapped_plans_give_heights(gpu, name):
    plans = _plans(*topo_case(name)[:2])
    _check(name, None, plans, reverse=True, calls=1)
    for kind in ("equal", "signed", "fractions") + (("ties", "peak_last") if name in LONG_ROWS else ()):
        _check(name, kind, plans, reverse=True, calls=1)


def test_symmetric_pattern_peels_exactly_the_isolated_vertices(gpu):
    cin, cout, _, _ = topo_case("symmetric")
    assert cout is None
    pin = _bool_plan(cin)
    level = _check("symmetric", "equal", (pin, None))[0]
    assert np.array_equal(np.flatnonzero(level != NONE), np.arange(3, 10))
    want = topo_expected("symmetric", "equal")
    w = topo_weights("symmetric", "equal")
    _compare(_topo(pin, pin, 10, w), want, 10)                         # plan_out == plan_in, said explicitly
    _compare(_topo(pin, _bool_plan(cin), 10, w), want, 10)             # a symmetric pattern given as two plans


def test_plan_without_entries_is_one_level(gpu):
    n = 64
    empty = _csr(n, [], [])
    general = capi.SpMVPlan(n, n, empty.adj_indptr, empty.adj_indices, empty.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        level, order, dist, parent, stats = _topo(general, None, n)
        assert np.all(level == 0) and np.array_equal(order, np.arange(n)) and stats == (n, 1, n, 1)
    level, order, dist, parent, stats = _topo(general, general, n)
    assert np.all(level == 0) and stats == (n, 1, n, 1)
    w = capi.DeviceBuffer.from_host(np.ones(1, np.float32))
    bufs = [capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32)) for _ in range(4)]
    assert general.topo(None, bufs[0], bufs[1], w, bufs[2], bufs[3]) == (n, 1, n, 1)
    capi.sync()
    got = [b.read(np.uint32, n + 64) for b in bufs]
    assert np.all(got[0][:n] == 0) and np.array_equal(got[1][:n], np.arange(n)) and np.all(got[2][:n] == 0) and np.all(got[3][:n] == NONE)
    assert all(np.all(g[n:] == GARBAGE) for g in got)


def test_refusals(gpu):
    cin, cout, _, _ = topo_case("bowtie")
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    want = topo_expected("bowtie")
    out = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))

    def still_works():
        _compare(_topo(pin, pout, n), want, n)

    def refused(a, b, needle):
        for _ in range(2):                                           # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                a.topo(b, out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value) and "gl_topo" in str(e.value), str(e.value)
        assert np.all(out.read(np.uint32, n) == GARBAGE), "a refused call writes nothing"
        still_works()
    general = capi.SpMVPlan(n, n, cin.adj_indptr, cin.adj_indices, cin.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, pout, "plan_in keeps no row copy")
    refused(pin, general, "plan_out keeps no row copy")
    refused(_bool_plan(cin, 0, n // 2), pout, "row shard")
    refused(pin, _bool_plan(cout, n // 2, n), "row shard")
    sh = permute_rows(cin, 77)
    assert not np.array_equal(sh.adj_indices, cin.adj_indices)
    refused(_bool_plan(sh), pout, "strictly ascending")              # unsorted rows
    refused(pin, _bool_plan(permute_rows(cout, 78)), "strictly ascending")
    ip = cin.adj_indptr.astype(np.int64)
    v = int(np.flatnonzero(np.diff(ip) >= 2)[0])
    dup = cin.copy()
    dup.adj_indices = cin.adj_indices.copy()
    dup.adj_indices[ip[v] + 1] = dup.adj_indices[ip[v]]              # a duplicate column
    refused(_bool_plan(dup), pout, "strictly ascending")
    z = cin.copy()
    z.adj_data = cin.adj_data.copy()
    z.adj_data[ip[v]] = 0.0                                          # a zero-valued entry: column 0xffffffff in the row copy
    refused(_bool_plan(z), pout, "strictly ascending")
    wide = io.CSRMatrix(n, n + 128, cin.adj_data, cin.adj_indices, cin.adj_indptr)
    refused(_bool_plan(wide), pout, "num_rows == num_cols")
    refused(pin, pin, "not symmetric")                               # plan_out == plan_in on an asymmetric pattern
    refused(pin, None, "io.simple_pattern prepares what it needs")   # (the same refusal: its hint)
    op = cout.adj_indptr.astype(np.int64)
    u = int(np.flatnonzero(np.diff(op) >= 1)[5])
    less = io.CSRMatrix(n, n, np.delete(cout.adj_data, op[u]), np.delete(cout.adj_indices, op[u]),
                        (op - (np.arange(n + 1) > u)).astype(np.uint32))
    refused(pin, _bool_plan(less), "not the transpose")
    small = _csr(128, [1], [0])
    refused(pin, _bool_plan(small), "not the transpose of plan_in: 128 and %d vertices" % n)
    # GL_ERR_INVALID_ARG: a NULL level, dist / parent without weights or the reverse, arrays that are one another
    w = capi.DeviceBuffer.from_host(topo_weights("bowtie", "equal"))
    a, b, c = (capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32)) for _ in range(3))
    for args in ((None,), (out, None, None, a, b), (out, None, None, a, None), (out, None, w, None, None), (out, None, w, a, None),
                 (out, None, w, None, b), (out, out), (out, a, w, a, b), (out, None, w, a, a), (out, None, w, out, b), (out, None, w, a, out),
                 (out, c, w, a, c)):
        with pytest.raises(capi.GraphLilyError) as e:
            pin.topo(pout, *args)
        assert e.value.code == capi.GL_ERR_INVALID_ARG, args
    for buf in (out, a, b, c):
        assert np.all(buf.read(np.uint32, n) == GARBAGE)
    still_works()                                                    # the verdict is cached per partner: the right one is accepted again


def _module(m):
    mod = M.SpMVModule(M.num_hbm_channels, 1024, 256)
    mod.set_semiring(M.LogicalSemiring)
    mod.set_mask_type(M.kNoMask)
    mod.set_up_runtime()
    mod.load_and_format_matrix(m.copy(), True)
    mod.send_matrix_host_to_device()
    return mod


def test_module_layer(gpu):
    name = "layered_2000_6000_perm"
    cin, cout, _, _ = topo_case(name)
    n = cin.num_rows
    a, b = _module(cin), _module(cout)
    w = topo_weights(name, "fractions")
    bufs = [capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32)) for _ in range(4)]
    stats = a.topo(b, bufs[0], bufs[1], capi.DeviceBuffer.from_host(w), bufs[2], bufs[3])
    capi.sync()
    _compare([x.read(np.uint32, n) for x in bufs] + [stats], topo_expected(name, "fractions"), n)
    stats = b.topo(a, bufs[0], None, capi.DeviceBuffer.from_host(transposed_weights(name, w)), bufs[2], bufs[3])
    capi.sync()
    _compare([bufs[0].read(np.uint32, n), None, bufs[2].read(np.uint32, n), bufs[3].read(np.uint32, n), stats], topo_expected(name, "fractions", True), n)
    s = _module(topo_case("symmetric")[0])
    stats = s.topo(None, bufs[0])
    capi.sync()
    assert np.array_equal(bufs[0].read(np.uint32, 10), topo_expected("symmetric")[0]) and stats[:3] == topo_expected("symmetric")[3]


def _driver(m, weighted=False):
    d = app.TopologicalOrder(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True, weighted)
    d.send_matrix_host_to_device()
    return d


def _path_sum(d, path, reverse):
    """the f32 running sum along the path, from the end whose dist is 0, over stored edges of the driver's graph"""
    g = d.graph_out_ if reverse else d.graph_
    total = np.float32(0.0)
    for i in range(len(path) - 1, 0, -1):
        v, u = int(path[i - 1]), int(path[i])                         # u is v's parent: an entry (v, u) of the pulling matrix
        row = g.adj_indices[g.adj_indptr[v]:g.adj_indptr[v + 1]]
        at = np.flatnonzero(row == u)
        assert at.size == 1, "the critical path uses (%d, %d), which is no stored edge" % (u, v)
        total = np.float32(total + g.adj_data[g.adj_indptr[v] + at[0]])
    return total


def test_driver_on_the_golden_file(gpu, golden_dir):
    path = os.path.join(golden_dir, GOLDEN)
    raw = io.load_csr_matrix_from_float_npz(path)
    d = _driver(path, weighted=True)
    n = d.n_
    assert (n, d.n_real_, d.symmetric_) == (256, 150, False) and d.out_ is not None
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(d.graph_.adj_indptr.astype(np.int64)))
    src = d.graph_.adj_indices.astype(np.int64)
    for reverse in (False, True):
        got = d.run(reverse=reverse, order=True)
        a, b = (dst, src) if reverse else (src, dst)
        level, dist, parent, (peeled, levels, widest) = topo_model(n, a, b, d.graph_.adj_data)
        assert got.dtype == np.uint32 and got.shape == (n,) and d.level_ is got and np.array_equal(got, level)
        assert np.array_equal(bits(d.dist_), bits(dist)) and np.array_equal(d.parent_, parent) and d.dist_.dtype == np.float32
        assert np.all(got[150:] == 0) and np.all(d.parent_[150:] == NONE) and np.all(d.dist_[150:] == 0)      # the padding: isolated
        real = level[:150] != NONE
        sizes = np.bincount(level[:150][real])
        assert d.num_peeled_ == int(real.sum()) == peeled - (n - 150) and not d.is_dag_ and np.array_equal(d.cyclic_, ~real)
        assert np.array_equal(d.level_sizes_, sizes) and d.num_levels_ == len(sizes) == levels and d.widest_ == sizes.max() and d.launches_ >= 2
        assert d.critical_length_ == float(dist[:150][real].max())
        order = d.order_.astype(np.int64)
        assert np.array_equal(order, np.flatnonzero(real)[np.lexsort((np.flatnonzero(real), level[:150][real]))])
        assert np.array_equal(d.position_[order], np.arange(order.size)) and np.all(d.position_[~real] == NONE)
        cp = d.critical_path()
        assert cp[0] == np.flatnonzero(real & (dist[:150] == np.float32(d.critical_length_)))[0] and parent[cp[-1]] == NONE
        assert bits(_path_sum(d, cp, reverse))[0] == bits(np.float32(d.critical_length_))[0]
        if not reverse:
            assert (d.num_peeled_, d.num_levels_) == (120, 7)
            assert app.validate_topological(raw, got, d.dist_, d.parent_, weighted=True) == 120 + n - 150
    d = _driver(path)                                                  # unweighted: the stored zero is no edge
    got = d.run()
    assert d.dist_ is None and d.parent_ is None and d.order_ is None and d.critical_length_ is None
    assert app.validate_topological(raw, got) == d.num_peeled_ + n - 150
    with pytest.raises(RuntimeError, match="weighted load first"):
        d.critical_path()


@pytest.mark.parametrize("weighted,reverse", [(0, 0), (1, 0), (1, 1)])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, golden_dir, weighted, reverse):
    build_cpp_driver("topo_driver.cpp")
    path = os.path.join(golden_dir, GOLDEN)
    r = subprocess.run([TOPO_DRIVER, path, str(tmp_path), str(weighted), str(reverse)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TopologicalOrder::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(path, bool(weighted))
    want = d.run(reverse=bool(reverse), order=True)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_level.bin"), dtype=np.uint32), want)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_order.bin"), dtype=np.uint32), d.order_)
    lines = ["symmetric: 0", "peeled: %d" % d.num_peeled_, "is_dag: 0", "levels: %d" % d.num_levels_, "widest: %d" % d.widest_]
    if weighted:
        assert np.array_equal(np.fromfile(str(tmp_path / "cpp_dist.bin"), dtype=np.uint32), bits(d.dist_))
        assert np.array_equal(np.fromfile(str(tmp_path / "cpp_parent.bin"), dtype=np.uint32), d.parent_)
        assert np.array_equal(np.fromfile(str(tmp_path / "cpp_path.bin"), dtype=np.uint32), d.critical_path())
        lines.append("critical_length: %.9g" % d.critical_length_)
    for line in lines:
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])


@pytest.mark.parametrize("name", ["bowtie_golden", "random_1000_1400"])
def test_condensation_of_the_strong_components_is_ordered(gpu, golden_dir, name):
    m = os.path.join(golden_dir, "scc_bowtie_csr_float32.npz") if name == "bowtie_golden" else scc_case(name)[0].copy()
    s = app.StronglyConnectedComponents(M.num_hbm_channels, 1024, 256)
    s.set_target("hw")
    s.set_up_runtime("unused.xclbin")
    s.load_and_format_matrix(m, True)
    s.send_matrix_host_to_device()
    labels = s.run()
    dag, rank = s.condensation()
    t = _driver(dag)                                                  # condensation()'s matrix goes straight in
    t.run(order=True)
    k = s.num_components_
    assert t.is_dag_ and t.num_peeled_ == k == t.n_real_ and t.order_.shape == (k,) and not t.cyclic_.any()
    src, dst = app._edges_of_pattern(s.graph_, s.n_real_)
    pos = t.position_[rank[labels[:s.n_real_]]].astype(np.int64)     # where every vertex's component stands
    assert np.all(pos[src] <= pos[dst]) and np.all((pos[src] < pos[dst]) == (labels[src] != labels[dst]))
    u = _driver(m)                                                     # the cyclic graph itself: what is peeled is in no cycle
    u.run()
    assert not u.is_dag_ and np.all(np.bincount(labels[:s.n_real_], minlength=s.n_real_)[labels[:s.n_real_]][~u.cyclic_] == 1)
