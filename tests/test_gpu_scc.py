"""GPU parity of the strongly connected components (gl_scc, SpMVPlan.scc, SpMVModule.scc, app.StronglyConnectedComponents,
graphlily::app::StronglyConnectedComponents) against the host model kept in tests/test_scc_cpu.py (scc_model, which that file checks
against scipy and the closed forms).  The labelling is unique and components, passes and trimmed are functions of (graph,
priorities), so every comparison is exact; the device's rounds are bounded by the model's synchronous ones.  Every test runs with
the default dealing of the rows and with scc_cut=0, the output buffer starts as garbage with 64 guard words behind it, and every
case is called twice on one pair of plans."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_cc_cpu import permute_rows
from test_kcore_cpu import _csr
from test_scc_cpu import CASES, N, SCC_DRIVER, build_cpp_driver, scc_case, scc_model

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef
GOLDEN = "scc_bowtie_csr_float32.npz"


@pytest.fixture(autouse=True, params=[None, 0], ids=["thread_per_short_row", "wavefront_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of the rows -- a thread reads the first scc_cut entries of its row, the
    wavefront takes over what is left -- and with scc_cut=0, which hands every row to the wavefront"""
    set_knob(monkeypatch, "scc_cut", request.param)


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _plans(cin, cout):
    return _bool_plan(cin), (None if cout is None else _bool_plan(cout))


def _scc(pin, pout, n, prio=None):
    """-> (labels, stats); the output buffer starts out as garbage, and a guard behind it must stay garbage"""
    out = capi.DeviceBuffer.from_host(np.full(n + 64, GARBAGE, np.uint32))
    dp = None if prio is None else capi.DeviceBuffer.from_host(np.ascontiguousarray(prio, np.uint32))
    stats = pin.scc(pout, out, dp)
    capi.sync()
    got = out.read(np.uint32, n + 64)
    assert len(stats) == 5 and 0xdeadbeefdeadbeef not in stats and np.all(got[n:] == GARBAGE)
    if dp is not None:
        assert np.array_equal(dp.read(np.uint32, n), np.asarray(prio, np.uint32)), "the priorities are read only"
    return got[:n], stats


def _check(name, plans=None):
    """labels, components, passes and trimmed are the model's, the rounds at most the model's; twice on one pair of plans"""
    cin, cout, prio, (lab, comps, passes, trimmed, rounds), _ = scc_case(name)
    pin, pout = _plans(cin, cout) if plans is None else plans
    first = None
    for _ in range(2):                                               # (the second time from the cached verdicts and scratch)
        got, stats = _scc(pin, pout, cin.num_rows, prio)
        assert np.array_equal(got, lab), "first difference at vertex %d" % int(np.flatnonzero(got != lab)[0])
        assert stats[:3] == (comps, passes, trimmed)
        assert passes <= stats[3] <= rounds
        assert stats[4] >= 2
        first = stats if first is None else first
        assert stats[:3] == first[:3]                                # (rounds and launches follow the hardware's schedule)
    return got, stats


@pytest.mark.parametrize("name", CASES)
def test_every_named_case(gpu, name):
    _check(name)


@pytest.mark.parametrize("name", ["cycle", "path", "chain_asc", "bowtie", "cliques_65", "random_1000_1400_perm"])
def test_results_do_not_depend_on_the_batch(gpu, monkeypatch, name):
    plans = _plans(*scc_case(name)[:2])
    _, default = _check(name, plans)
    set_knob(monkeypatch, "scc_batch", 1)
    _, single = _check(name, plans)
    assert single[:3] == default[:3]
    set_knob(monkeypatch, "scc_batch", 7)
    set_knob(monkeypatch, "scc_grid", 1)
    assert _check(name, plans)[1][:3] == default[:3]


def test_symmetric_pattern_equals_cc_labels(gpu):
    cin, cout, _, (lab, comps, _, _, _), _ = scc_case("symmetric")
    assert cout is None
    pin = _bool_plan(cin)
    got, stats = _check("symmetric", (pin, None))
    out = capi.DeviceBuffer.from_host(np.full(N, GARBAGE, np.uint32))
    pin.cc_labels(out)
    capi.sync()
    assert np.array_equal(out.read(np.uint32, N), got)
    assert np.array_equal(_scc(pin, pin, N)[0], got)                  # plan_out == plan_in, said explicitly
    assert np.array_equal(_scc(pin, _bool_plan(cin), N)[0], got)      # a symmetric pattern given as two plans


@pytest.mark.parametrize("name", ["bowtie", "random_300_500", "random_300_1500", "random_1000_1400"])
def test_labels_do_not_depend_on_the_priorities(gpu, name):
    cin, cout, _, (lab, comps, _, _, _), (src, dst) = scc_case(name)
    n = cin.num_rows
    plans = _plans(cin, cout)
    degrees = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    for order in ("natural", "random", "largest_first"):
        prio = io.coloring_priorities(degrees, order, 3)
        got, stats = _scc(*plans, n, prio)
        want = scc_model(n, src, dst, prio)
        assert np.array_equal(got, lab) and stats[:3] == want[1:4] and want[1] == comps and stats[3] <= want[4], order


def test_chain_takes_one_pass_under_priorities_descending_along_it(gpu):
    assert _check("chain_asc")[1][1] == 40 and _check("chain_desc")[1][1] == 1
    assert _check("chain_asc_prio")[1][1] == 1


def test_plan_without_entries_writes_iota(gpu):
    empty = _csr(N, [], [])
    general = capi.SpMVPlan(N, N, empty.adj_indptr, empty.adj_indices, empty.adj_data, 0, N, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        got, stats = _scc(general, None, N)
        assert np.array_equal(got, np.arange(N)) and stats == (N, 0, 0, 0, 0)     # (no launch beyond the one that numbers the labels)
    got, stats = _scc(general, general, N, np.arange(N)[::-1])
    assert np.array_equal(got, np.arange(N)) and stats == (N, 0, 0, 0, 0)


def test_refusals(gpu):
    cin, cout, _, (lab, _, _, _, _), _ = scc_case("bowtie")
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    out = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))

    def still_works():
        assert np.array_equal(_scc(pin, pout, n)[0], lab)

    def refused(a, b, needle):
        for _ in range(2):                                           # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                a.scc(b, out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
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
    refused(pin, None, "io.simple_pattern prepares what it needs")     # (the same refusal: its hint)
    # plan_out that is not the transpose: one entry removed
    op = cout.adj_indptr.astype(np.int64)
    u = int(np.flatnonzero(np.diff(op) >= 1)[5])
    less = io.CSRMatrix(n, n, np.delete(cout.adj_data, op[u]), np.delete(cout.adj_indices, op[u]),
                        (op - (np.arange(n + 1) > u)).astype(np.uint32))
    refused(pin, _bool_plan(less), "not the transpose")
    # ... and a DIFFERENT graph on the same vertices with as many entries: every vertex renamed by a rotation
    src, dst = scc_case("bowtie")[4]
    other = io.simple_pattern(_csr(n, (src + 1) % n, (dst + 1) % n))[0]      # row v: the successors, of the rotated graph
    assert other.nnz == cout.nnz and not np.array_equal(other.adj_indices, cout.adj_indices)
    refused(pin, _bool_plan(other), "not the transpose")
    with pytest.raises(capi.GraphLilyError) as e:
        pin.scc(pout, None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    with pytest.raises(capi.GraphLilyError) as e:
        pin.scc(pout, out, out)                                      # d_prio == d_label
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    assert np.all(out.read(np.uint32, n) == GARBAGE)
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
    cin, cout, _, (lab, comps, passes, trimmed, rounds), _ = scc_case("bowtie")
    a, b = _module(cin), _module(cout)
    out = capi.DeviceBuffer.from_host(np.full(N, GARBAGE, np.uint32))
    stats = a.scc(b, out)
    capi.sync()
    assert np.array_equal(out.read(np.uint32, N), lab) and stats[:3] == (comps, passes, trimmed) and stats[3] <= rounds
    sym = scc_case("symmetric")
    s = _module(sym[0])
    stats = s.scc(None, out)
    capi.sync()
    assert np.array_equal(out.read(np.uint32, N), sym[3][0]) and stats[:3] == sym[3][1:4]


def _driver(m):
    d = app.StronglyConnectedComponents(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True)
    d.send_matrix_host_to_device()
    return d


def test_driver_on_the_golden_bowtie(gpu, golden_dir):
    """tests/golden/scc_bowtie_csr_float32.npz: the bow tie of tests/test_scc_cpu.py on 442 vertices renamed by a seeded
    permutation -- an IN tree of 100, a core cycle of 200 with two chords, an OUT tree of 100, two tendrils of 20 and a two-cycle --
    with a loop, a zero-valued entry and its rows stored unsorted"""
    path = os.path.join(golden_dir, GOLDEN)
    raw = io.load_csr_matrix_from_float_npz(path)
    assert (raw.num_rows, raw.num_cols) == (442, 442)
    d = _driver(path)
    n = d.n_
    assert (n, d.n_real_, d.symmetric_) == (512, 442, False) and d.out_ is not None and d.graph_.nnz == d.graph_out_.nnz == 444
    src, dst = app._edges_of_pattern(d.graph_, n)
    for order in ("largest_first", "natural", "random"):
        got = d.run(order=order, seed=2)
        prio = io.coloring_priorities(d.degrees_, order, 2)
        assert (prio is None and d.priorities_ is None) or np.array_equal(d.priorities_, prio)
        lab, comps, passes, trimmed, rounds = scc_model(n, src, dst, prio)
        assert got.dtype == np.uint32 and got.shape == (n,) and d.labels_ is got and np.array_equal(got, lab)
        assert (d.num_components_, d.passes_, d.trimmed_) == (comps - (n - 442), passes, trimmed - (n - 442))
        assert d.passes_ <= d.rounds_ <= rounds and d.launches_ >= 2
        assert (d.num_components_, d.largest_component_, d.is_dag_) == (442 - 200 - 2 + 2, 200, False)
        assert app.validate_strong_components(raw, got) == comps
        assert np.array_equal(got[442:], np.arange(442, n))
        assert int(d.component_sizes_.sum()) == 442 and sorted(d.component_sizes_.tolist())[-2:] == [2, 200]
        assert np.array_equal(d.component_labels_, np.unique(got[:442]))
    dag, rank = d.condensation()
    k = d.num_components_
    assert (dag.num_rows, dag.num_cols) == (k, k) and rank.shape == (442,)
    assert np.array_equal(np.flatnonzero(rank != 0xFFFFFFFF), d.component_labels_) and np.array_equal(rank[d.component_labels_], np.arange(k))
    # every edge between two components is an entry, every entry is such an edge, and the result is a DAG
    a, b = rank[got[src]].astype(np.int64), rank[got[dst]].astype(np.int64)
    want = np.unique(b[a != b] * k + a[a != b])
    rows = np.repeat(np.arange(k), np.diff(dag.adj_indptr.astype(np.int64)))
    assert np.array_equal(rows * k + dag.adj_indices, want) and dag.nnz == 444 - 202 - 2
    assert app.validate_strong_components(dag, np.arange(k)) == k
    dd = _driver(dag)                                                # ... which the device finds to be one
    assert np.array_equal(dd.run()[:k], np.arange(k)) and dd.is_dag_ and dd.passes_ == 0 and dd.trimmed_ == k
    with pytest.raises(ValueError, match="priorities of shape"):
        d.run(priorities=np.arange(5))
    assert np.array_equal(d.run(priorities=np.arange(442)[::-1].copy()), got)


@pytest.mark.parametrize("order,seed", [("largest_first", 0), ("natural", 0), ("random", 4)])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, golden_dir, order, seed):
    build_cpp_driver("scc_driver.cpp")
    path = os.path.join(golden_dir, GOLDEN)
    r = subprocess.run([SCC_DRIVER, path, str(tmp_path), order, str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "StronglyConnectedComponents::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(path)
    want = d.run(order=order, seed=seed)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_label.bin"), dtype=np.uint32), want)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    for line in ("symmetric: 0", "components: %d" % d.num_components_, "largest: %d" % d.largest_component_, "is_dag: 0",
                 "passes: %d" % d.passes_, "trimmed: %d" % d.trimmed_, "checksum: %d" % checksum):
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])
