"""GPU parity of the betweenness centrality (gl_bc_accumulate, SpMVPlan.bc_accumulate, app.BetweennessCentrality,
graphlily::app::BetweennessCentrality) against the host restatement of the definition (app.betweenness_by_levels, checked against
networkx and the closed forms in tests/test_bc_cpu.py) and against closed forms.  Unless a case says otherwise the levels come
from a host BFS and are uploaded, so the kernels are tested apart from the BFS schedule, and outputs the call must write start out
as garbage.  The tolerance is the derived bound of tests/test_bc_cpu.py -- 4 (D (longest row + 4) + sources) 2^-53 from the case's
own depth, longest row and source count -- plus equal zero patterns; path counts are compared exactly where a case says so."""
import functools
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_cc_cpu import permute_rows
from test_kcore_cpu import _csr
from test_bc_cpu import (BC_DRIVER, assert_close, bipartite_graph, bound_of, build_cpp_driver, cycle_graph, diamond_chain,
                         host_bc, longest_row, many_sample, nx_bc, path_graph, prepared, save_npz, star_graph)

pytestmark = pytest.mark.gpu

GARBAGE = np.full(1, 0xdeadbeefdeadbeef, np.uint64).view(np.float64)[0]


def _pad128(n):
    return (n + 127) // 128 * 128


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _plans(cin, cout):
    pin = _bool_plan(cin)
    return pin, (pin if cout is None else _bool_plan(cout))


def _bc(pin, pout, level, scale=1.0, accumulate=False, bc0=None, sigma=True):
    """-> (bc, sigma or None, stats); what the call must write starts out as garbage"""
    n = level.shape[0]
    lev = capi.DeviceBuffer.from_host(np.ascontiguousarray(level, np.float32))
    bc = capi.DeviceBuffer.from_host(np.full(n, GARBAGE) if bc0 is None else np.ascontiguousarray(bc0, np.float64))
    sg = capi.DeviceBuffer.from_host(np.full(n, GARBAGE)) if sigma else None
    stats = pin.bc_accumulate(pout, lev, bc, scale, accumulate, sg)
    assert len(stats) == 4 and 0xdeadbeef not in stats
    return bc.read(np.float64, n), (sg.read(np.float64, n) if sigma else None), stats


def _levels(cin, cout, sources, n):
    return app._bfs_levels_of(app._pattern_as_scipy(cin if cout is None else cout, n), sources, n)


def _host(cin, cout, level):
    """-> (sigma, bc of one call with scale 1 and accumulate 0, orphans)"""
    sigma, delta = app.betweenness_by_levels(cin, cout, level)
    return sigma, np.where(level >= 2, delta, 0.0), int(np.count_nonzero((level >= 2) & (sigma == 0)))


def _all_sources(m, sources, scale):
    """the kernel summed over single-source searches from host levels -> (bc, deepest level)"""
    cin, cout, _ = app._bc_patterns(m, None)
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    A = app._pattern_as_scipy(cin if cout is None else cout, n)
    lev = capi.DeviceBuffer(4 * n)
    bc = capi.DeviceBuffer.from_host(np.full(n, GARBAGE))
    depth = 1
    for i, s in enumerate(sources):
        level = app._bfs_levels_of(A, [s], n)
        lev.write(level)
        st = pin.bc_accumulate(pout, lev, bc, scale, i > 0)
        assert st[0] == int(level.max()) and st[1] == np.count_nonzero(level) and st[2:] == (0, 0)
        depth = max(depth, st[0])
    return bc.read(np.float64, n), depth, longest_row(cin, cout)


def _driver(m, directed=None):
    d = app.BetweennessCentrality(M.num_hbm_channels, 1024, 512, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True, directed)
    d.send_matrix_host_to_device()
    return d


def _fixed_sources(name, raw):
    if name == "line_8":
        return list(range(raw.num_rows))
    return [int(s) for s in np.random.default_rng(17).choice(raw.num_rows, 8, replace=False)]


def _far_source(name):
    """the first of the fixed sources that reaches more than a thousand vertices (some of them are isolated)"""
    sources, _, _, reached, _ = _reference(name)
    return next(s for s, r in zip(sources, reached) if r > 1000)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """-> (sources, bc of the host restatement with the driver's scale, depths, reached counts, bound); shared, never written"""
    raw, m, cin, cout, directed = prepared(name)
    sources = _fixed_sources(name, raw)
    scale = app._bc_scale(raw.num_rows, len(sources), False, directed)
    want, depths, reached = host_bc(cin, cout, sources, cin.num_rows, scale)
    want.setflags(write=False)
    return sources, want, depths, reached, bound_of(max(depths), longest_row(cin, cout), len(sources))


@pytest.mark.parametrize("name", ["uniform_10K_10", "rmat_20K", "rmat_sym_50K", "gplus_small", "line_8"])
def test_drivers(gpu, name):
    raw, m, cin, cout, directed = prepared(name)
    sources, want, depths, reached, bound = _reference(name)
    d = _driver(raw)
    got = d.run(sources)
    assert got.dtype == np.float64 and got.shape == (m.num_rows,) and d.bc_ is got and d.n_real_ == raw.num_rows
    assert d.directed_ == directed and (d.out_ is not None) == directed and (name != "rmat_20K" or directed)
    assert_close(got, want, bound, name)
    assert not got[raw.num_rows:].any()
    assert d.depths_ == depths and d.reached_ == reached and d.sources_ == sources
    assert d.orphans_ == 0 and d.overflowed_ == []
    assert app.validate_betweenness(raw, got, sources) <= bound
    if name == "line_8":
        assert_close(got[:8], nx_bc(cin, cout, m.num_rows, False, nodes=range(8))[:8], bound, "networkx")
        norm = d.run(normalized=True)                                # (sources=None: all real vertices)
        assert_close(norm[:8], nx_bc(cin, cout, m.num_rows, True, nodes=range(8))[:8], bound, "networkx, normalised")
        assert not norm[8:].any() and app.validate_betweenness(raw, norm, normalized=True) <= bound


def test_driver_on_an_empty_graph_launches_nothing(gpu):
    raw = prepared("eye_10")[0]
    d = _driver(raw)
    assert d.empty_ and d.get_nnz() == 0
    got = d.run()
    assert got.shape == (d.n_,) and not got.any() and d.depths_ == [1] * 10 and d.reached_ == [1] * 10
    assert app.validate_betweenness(raw, got) == 0.0
    # the C ABI on a plan without entries: bc as accumulate says, sigma and the stats from the levels
    n = 256
    e = _csr(n, [], [])
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    level = np.zeros(n, np.float32)
    level[[3, 9]] = 1
    for _ in range(2):
        bc, sigma, stats = _bc(empty, None, level)
        assert not bc.any() and stats == (1, 2, 0, 0) and np.array_equal(sigma, (level == 1).astype(np.float64))
    keep = np.random.default_rng(1).random(n)
    bc, _, stats = _bc(empty, None, np.zeros(n, np.float32), accumulate=True, bc0=keep)
    assert np.array_equal(bc, keep) and stats == (0, 0, 0, 0)


def test_driver_on_whole_components_of_many_against_networkx(gpu):
    """all the sources of a sample of whole components (test_bc_cpu.many_sample says why not all 90 789), the one-way edges read
    as undirected: the sampled components' values are the all-sources values of the whole graph up to networkx's n / k"""
    raw, m, _, _, _ = prepared("many")
    sources, comps = many_sample()
    sym = io.symmetrize_simple(m)[0]
    n, k = sym.num_rows, len(sources)
    d = _driver(raw, directed=False)
    assert d.directed_ is False and d.out_ is None
    got = d.run(sources)
    want, depths, reached = host_bc(sym, None, sources, n, app._bc_scale(raw.num_rows, k, False, False))
    bound = bound_of(max(depths), longest_row(sym, None), k)
    assert_close(got, want, bound, "many")
    assert d.depths_ == depths and d.reached_ == reached and d.orphans_ == 0
    assert app.validate_betweenness(raw, got, sources, directed=False) <= bound
    # the one-way edges as they are stored: a directed graph on two plans, against the host restatement of the same reading
    _, _, cin, cout, directed = prepared("many")
    two = _driver(raw)
    assert directed and two.directed_ is True and two.out_ is not None
    got2 = two.run(sources)
    want2, depths2, reached2 = host_bc(cin, cout, sources, n, app._bc_scale(raw.num_rows, k, False, True))
    assert_close(got2, want2, bound_of(max(depths2), longest_row(cin, cout), k), "many, directed")
    assert two.depths_ == depths2 and two.reached_ == reached2 and two.orphans_ == 0
    norm = d.run(sources, normalized=True)
    for c in comps:
        ref = nx_bc(sym, None, n, False, nodes=c.tolist())[c]        # = 0.5 x the sum over the component's sources
        assert_close(got[c], ref * raw.num_rows / k, bound, "networkx, component of %d" % c.size)
        assert_close(norm[c], ref * 2.0 * app._bc_scale(raw.num_rows, k, True, False), bound, "networkx normalised, component of %d" % c.size)


def test_truncated_search_is_run_again_deeper(gpu):
    m, want = path_graph(300)
    d = _driver(m)
    assert d.n_ == 384 and d.directed_ is False
    got = d.run(depth_hint=4)
    assert_close(got, np.concatenate([want, np.zeros(84)]), bound_of(300, 2, 300), "P_300")
    assert d.depths_[0] == d.depths_[-1] == 300 and max(d.depths_) == 300 and d.depths_[150] == 151 and set(d.reached_) == {300}


@pytest.mark.parametrize("cut", [0, 1 << 40])
@pytest.mark.parametrize("case", ["P_9", "C_8", "C_9", "K_70_300"])
def test_closed_forms_through_the_kernel(gpu, monkeypatch, case, cut):
    set_knob(monkeypatch, "bc_cut", cut)
    kind, *k = case.split("_")
    k = [int(x) for x in k]
    n = _pad128(sum(k))
    m, want = {"P": path_graph, "C": cycle_graph}[kind](k[0], n) if kind != "K" else bipartite_graph(k[0], k[1], n)
    got, depth, longest = _all_sources(m, range(sum(k)), 0.5)
    assert_close(got, want, bound_of(depth, longest, sum(k)), case)
    if kind == "K":                                                  # path counts at distance 2: the size of the other side, exactly
        cin, cout, _ = app._bc_patterns(m, None)
        pin, pout = _plans(cin, cout)
        for s, other in ((0, 300.0), (70, 70.0)):
            level = _levels(cin, cout, [s], n)
            _, sigma, stats = _bc(pin, pout, level)
            assert stats == (3, 370, 0, 0) and np.all(sigma[level == 3] == other) and np.all(sigma[level == 2] == 1.0)


@pytest.mark.parametrize("cut", [0, 8, 1 << 40])
def test_star_whose_centre_row_spans_many_wavefront_steps(gpu, monkeypatch, cut):
    set_knob(monkeypatch, "bc_cut", cut)
    n, centre = 5120, 11
    m, _ = star_graph(5000, n, centre)
    cin, cout, _ = app._bc_patterns(m, None)
    pin, pout = _plans(cin, cout)
    for s in (centre, 4000):
        level = _levels(cin, cout, [s], n)
        hs, hbc, _ = _host(cin, cout, level)
        for _ in range(2):
            bc, sigma, stats = _bc(pin, pout, level)
            assert stats == (2 if s == centre else 3, 5001, 0, 0) and np.array_equal(sigma, hs)
            assert_close(bc, hbc, bound_of(stats[0], 5000, 1), "star from %d" % s)
        assert bc[centre] == (0.0 if s == centre else 4999.0) and np.count_nonzero(bc) == (0 if s == centre else 1)


def test_exact_path_counts_on_a_deep_chain_of_diamonds(gpu):
    k = 1000
    n = _pad128(3 * k + 1)
    m, _, from0 = diamond_chain(k, n)
    cin, cout, directed = app._bc_patterns(m, None)
    assert directed
    pin, pout = _plans(cin, cout)
    level = _levels(cin, cout, [0], n)
    bc, sigma, stats = _bc(pin, pout, level)
    assert stats == (2 * k + 1, 3 * k + 1, 0, 0)
    assert np.array_equal(sigma[0:3 * k + 1:3], 2.0 ** np.arange(k + 1))         # sums of equal powers of two are exact
    assert np.array_equal(sigma[1:3 * k:3], 2.0 ** np.arange(k)) and np.array_equal(sigma[2:3 * k:3], 2.0 ** np.arange(k))
    assert not sigma[3 * k + 1:].any()
    assert_close(bc, from0, bound_of(2 * k + 1, 2, 1), "diamonds from 0")


def test_overflowing_path_counts_gate_the_backward_sweep(gpu):
    k = 1100
    n = _pad128(3 * k + 1)
    m, _, _ = diamond_chain(k, n)
    cin, cout, _ = app._bc_patterns(m, None)
    pin, pout = _plans(cin, cout)
    level = _levels(cin, cout, [0], n)
    keep = np.random.default_rng(3).random(n)
    bc, sigma, stats = _bc(pin, pout, level, accumulate=True, bc0=keep)
    assert stats[:3] == (2 * k + 1, 3 * k + 1, 0) and stats[3] == 3 * (k - 1024) + 1 == np.count_nonzero(np.isinf(sigma))
    assert np.array_equal(bc, keep), "nothing is added"
    assert not np.isnan(sigma).any() and np.array_equal(sigma[0:3 * 1023 + 1:3], 2.0 ** np.arange(1024))
    bc, sigma2, stats2 = _bc(pin, pout, level)
    assert not bc.any() and stats2 == stats and np.array_equal(sigma2, sigma)
    d = _driver(m)
    with pytest.warns(RuntimeWarning, match=r"from \[0\] overflowed"):
        got = d.run([0, 3 * 1050], depth_hint=4096)
    assert d.overflowed_ == [0] and d.depths_ == [2 * k + 1, 2 * (k - 1050) + 1] and np.all(np.isfinite(got))
    want, _, _ = host_bc(cin, cout, [3 * 1050], n)                   # (directed, not normalised: networkx rescales nothing)
    assert_close(got, want, bound_of(2 * k + 1, 2, 2), "the source that did not overflow")


def test_levels_that_are_no_bfs_result(gpu):
    # P_9 from vertex 0, vertex 4 two levels too deep: 5 loses its only predecessor, and everybody behind it
    m, _ = path_graph(9, 128)
    cin, cout, _ = app._bc_patterns(m, None)
    pin, pout = _plans(cin, cout)
    level = _levels(cin, cout, [0], 128)
    level[4] += 2
    hs, hbc, orphans = _host(cin, cout, level)
    bc, sigma, stats = _bc(pin, pout, level)
    assert orphans > 0 and stats == (9, 9, orphans, 0) and np.array_equal(sigma, hs) and np.all(np.isfinite(bc))
    assert_close(bc, hbc, bound_of(9, 2, 1), "P_9")
    raw, mm, cin, cout, _ = prepared("uniform_10K_10")
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    level = _levels(cin, cout, [5], n).copy()
    v = int(np.flatnonzero(level == 3)[7])
    level[v] += 2
    hs, hbc, orphans = _host(cin, cout, level)
    bc, sigma, stats = _bc(pin, pout, level)
    assert stats == (int(level.max()), np.count_nonzero(level), orphans, 0) and np.all(np.isfinite(bc))
    assert_close(sigma, hs, bound_of(stats[0], longest_row(cin, cout), 1), "sigma")
    assert_close(bc, hbc, bound_of(stats[0], longest_row(cin, cout), 1), "uniform_10K_10")
    bad = level.copy()
    bad[3] = 2.5                                                     # not a level at all
    with pytest.raises(capi.GraphLilyError) as e:
        _bc(pin, pout, bad)
    assert e.value.code == capi.GL_ERR_INVALID_ARG


def test_two_sources_at_level_one(gpu):
    raw, m, cin, cout, directed = prepared("rmat_sym_50K")
    assert not directed
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    deg = np.diff(cin.adj_indptr.astype(np.int64))
    s = np.flatnonzero(deg > 0)[[10, 2000]]
    level = _levels(cin, cout, s, n)
    hs, hbc, orphans = _host(cin, cout, level)
    bc, sigma, stats = _bc(pin, pout, level, scale=0.25)
    bound = bound_of(int(level.max()), int(deg.max()), 2)
    assert stats == (int(level.max()), np.count_nonzero(level), 0, 0) and orphans == 0 and np.count_nonzero(level == 1) == 2
    assert_close(sigma, hs, bound, "sigma")
    assert_close(bc, 0.25 * hbc, bound, "bc")


def test_determinism(gpu):
    raw, m, cin, cout, _ = prepared("gplus_small")
    n = cin.num_rows
    level = _levels(cin, cout, [_far_source("gplus_small")], n)
    pin, pout = _plans(cin, cout)
    bc1, s1, st1 = _bc(pin, pout, level)
    bc2, s2, st2 = _bc(pin, pout, level)
    fresh_in, fresh_out = _plans(cin, cout)
    bc3, s3, st3 = _bc(fresh_in, fresh_out, level)
    assert st1 == st2 == st3 and st1[1] > 1000 and bc1.max() > 0
    assert np.array_equal(bc1, bc2) and np.array_equal(s1, s2) and np.array_equal(bc1, bc3) and np.array_equal(s1, s3)
    bc4, none, st4 = _bc(pin, pout, level, sigma=False)              # d_sigma = NULL: the plan's scratch
    assert none is None and st4 == st1 and np.array_equal(bc4, bc1)


def test_accumulate_and_scale(gpu):
    raw, m, cin, cout, _ = prepared("uniform_10K_10")
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    la, lb = _levels(cin, cout, [11], n), _levels(cin, cout, [4242], n)
    ra, _, sa = _bc(pin, pout, la)
    rb, _, sb = _bc(pin, pout, lb)
    start = 1.0 + np.random.default_rng(9).random(n)
    one, _, _ = _bc(pin, pout, la, accumulate=True, bc0=start)
    assert np.array_equal(one[la < 2], start[la < 2]), "unreached vertices and the source are untouched"
    assert (la < 2).sum() >= n - raw.num_rows + 1 and not np.array_equal(one, start)
    both, _, _ = _bc(pin, pout, lb, scale=0.5, accumulate=True, bc0=one)
    assert_close(both, start + ra + 0.5 * rb, bound_of(max(sa[0], sb[0]), longest_row(cin, cout), 2), "weighted sum")
    assert np.array_equal(both[(la < 2) & (lb < 2)], start[(la < 2) & (lb < 2)])
    neg, _, _ = _bc(pin, pout, la, scale=-2.0)
    assert np.array_equal(neg, -2.0 * ra)                            # (a power of two scales exactly)


@pytest.mark.parametrize("cut", [8, 0])
def test_entry_list_with_a_nonzero_first_offset(gpu, monkeypatch, cut):
    """the C ABI accepts a whole-matrix CSR whose indptr[0] is k != 0: the row copy's offsets then count from the caller's entry
    list while its indices start at entry k (csr_nz_base); here on both plans, with different k, on the thread's and on the
    wavefront's path"""
    set_knob(monkeypatch, "bc_cut", cut)
    raw, m, cin, cout, directed = prepared("rmat_20K")
    assert directed
    n = cin.num_rows
    level = _levels(cin, cout, [_far_source("rmat_20K")], n)
    pin, pout = _plans(cin, cout)
    want_bc, want_sigma, want_stats = _bc(pin, pout, level)
    assert want_stats[1] > 1000

    def shifted(c, k):
        junk = np.full(k, n - 1, np.uint32)                          # (entries in front of row 0 that belong to no row)
        p = capi.SpMVPlan(n, n, c.adj_indptr + np.uint32(k), np.concatenate([junk, c.adj_indices]),
                          np.concatenate([np.ones(k, np.float32), c.adj_data]), 0, n, flags=capi.GL_PLAN_BOOLEAN)
        assert p.info()["layout"] == "boolean" and p.info()["nnz"] == c.nnz
        return p
    a, b = shifted(cin, 77), shifted(cout, 5)
    for _ in range(2):
        bc, sigma, stats = _bc(a, b, level)
        assert stats == want_stats and np.array_equal(sigma, want_sigma) and np.array_equal(bc, want_bc)
    assert np.array_equal(_bc(a, pout, level)[0], want_bc)           # (a shifted plan with a plain partner)


def test_refusals(gpu):
    raw, m, cin, cout, directed = prepared("rmat_20K")
    n = cin.num_rows
    pin, pout = _plans(cin, cout)
    level = _levels(cin, cout, [_far_source("rmat_20K")], n)
    want = _bc(pin, pout, level)[0]
    lev = capi.DeviceBuffer.from_host(level)
    out = capi.DeviceBuffer.from_host(np.full(n, GARBAGE))

    def still_works():
        assert np.array_equal(_bc(pin, pout, level)[0], want)

    def refused(a, b, needle):
        for _ in range(2):                                           # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                a.bc_accumulate(b, lev, out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
        assert np.all(out.read(np.uint64, n) == np.uint64(0xdeadbeefdeadbeef)), "a refused call writes nothing"
        still_works()
    general = capi.SpMVPlan(n, n, cin.adj_indptr, cin.adj_indices, cin.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, pout, "plan_in keeps no row copy")
    refused(pin, general, "plan_out keeps no row copy")
    refused(_bool_plan(cin, 0, n // 2), pout, "row shard")
    refused(pin, _bool_plan(cout, n // 2, n), "row shard")
    sh = permute_rows(cin, 77)
    assert not np.array_equal(sh.adj_indices, cin.adj_indices)
    refused(_bool_plan(sh), pout, "strictly ascending")
    refused(pin, _bool_plan(permute_rows(cout, 78)), "strictly ascending")
    ip = cin.adj_indptr.astype(np.int64)
    v = int(np.flatnonzero(np.diff(ip) >= 2)[0])
    dup = cin.copy()
    dup.adj_indices = cin.adj_indices.copy()
    dup.adj_indices[ip[v] + 1] = dup.adj_indices[ip[v]]              # a duplicate column
    refused(_bool_plan(dup), pout, "strictly ascending")
    z = cin.copy()
    z.adj_data = cin.adj_data.copy()
    # a column >= n: a square plan cannot be created with one (plan creation refuses it), except through a zero-valued entry,
    # which the row copy stores as column 0xffffffff
    z.adj_data[ip[v]] = 0.0
    refused(_bool_plan(z), pout, "strictly ascending")
    wide = io.CSRMatrix(n, n + 128, cin.adj_data, cin.adj_indices, cin.adj_indptr)
    refused(_bool_plan(wide), pout, "num_rows == num_cols")
    # plan_out that is not the transpose: one entry removed; one entry moved to another column of its row
    op = cout.adj_indptr.astype(np.int64)
    u = int(np.flatnonzero(np.diff(op) >= 1)[5])
    less = io.CSRMatrix(n, n, np.delete(cout.adj_data, op[u]), np.delete(cout.adj_indices, op[u]),
                        (op - (np.arange(n + 1) > u)).astype(np.uint32))
    refused(pin, _bool_plan(less), "not the transpose")
    moved = cout.copy()
    moved.adj_indices = cout.adj_indices.copy()
    row = cout.adj_indices[op[u]:op[u + 1]]
    free = int(np.setdiff1d(np.arange(n, dtype=np.int64), np.concatenate([row, [u]]))[0])
    moved.adj_indices[op[u]:op[u + 1]] = np.sort(np.concatenate([row[:-1], [free]])).astype(np.uint32)
    assert moved.nnz == cout.nnz and not np.array_equal(moved.adj_indices, cout.adj_indices)
    refused(pin, _bool_plan(moved), "not the transpose")
    refused(pin, pin, "not symmetric")                               # plan_out == plan_in on an asymmetric pattern
    refused(pin, None, "not symmetric")
    refused(pout, pout, "not symmetric")
    with pytest.raises(capi.GraphLilyError) as e:
        pin.bc_accumulate(pout, lev, None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    with pytest.raises(capi.GraphLilyError) as e:
        pin.bc_accumulate(pout, lev, out, sigma=out)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    # the verdict is cached per partner: the right one is accepted again after a wrong one
    still_works()
    sym = io.symmetrize_simple(m)[0]
    ps = _bool_plan(sym)
    ls = _levels(sym, None, [_far_source("rmat_20K")], n)
    a = _bc(ps, None, ls)
    b = _bc(ps, _bool_plan(sym), ls)                                 # a symmetric pattern given as two plans
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["uniform_10K_10", "rmat_20K"])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, name):
    build_cpp_driver("bc_driver.cpp")
    raw, m, cin, cout, directed = prepared(name)
    sources = _fixed_sources(name, raw)[:4]
    path = str(tmp_path / (name + "_csr_float32.npz"))
    save_npz(raw, path)
    r = subprocess.run([BC_DRIVER, path, str(tmp_path)] + [str(s) for s in sources], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BetweennessCentrality::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "cpp_bc.bin"), dtype=np.float64)
    d = _driver(raw)
    want = d.run(sources)
    assert np.array_equal(got, want)
    assert "directed: %d\n" % int(directed) in r.stdout
    assert "depths: %s\n" % " ".join(str(x) for x in d.depths_) in r.stdout
    assert "reached: %s\n" % " ".join(str(x) for x in d.reached_) in r.stdout and "overflowed: 0\n" in r.stdout
