"""GPU parity of the graph colouring (gl_color, SpMVPlan.color, SpMVModule.color, app.GraphColoring, graphlily::app::GraphColoring):
the colouring is a pure function of (graph, priorities), so every comparison is np.array_equal against the host statement of the
definitions (greedy_by_priority, tests/test_coloring_cpu.py) or a closed form, and rounds and widest are compared with the host's
values too.  No tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_cc_cpu import permute_rows
from test_coloring_cpu import (COLORING_DRIVER, ORDERS, RECORDS, build_cpp_driver, graph, greedy_by_priority, reference, save_npz,
                               summary)
from test_gpu_kcore import _bool_plan, _clique_edges, _graph, _sorted_rows
from test_kcore_cpu import RECORDS as KCORE_RECORDS, _csr

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef
NAMES = ["uniform_10K_10", "rmat_20K", "rmat_sym_50K", "gplus_small", "line_8", "eye_10", "many"]


def _driver(m):
    gc = app.GraphColoring(M.num_hbm_channels, 1024, 256)
    gc.set_target("hw")
    gc.set_up_runtime("unused.xclbin")
    gc.load_and_format_matrix(m, True)
    gc.send_matrix_host_to_device()
    return gc


def _color(plan, n, prio=None):
    """-> (colours, stats); the colours start out as garbage: the call writes every word itself"""
    out = capi.DeviceBuffer.from_host(np.full(n, GARBAGE, np.uint32))
    dp = None if prio is None else capi.DeviceBuffer.from_host(np.ascontiguousarray(prio, dtype=np.uint32))
    stats = plan.color(dp, out)
    assert len(stats) == 4 and all(s < (1 << 32) for s in stats)
    if dp is not None:
        assert np.array_equal(dp.read(np.uint32, n), np.asarray(prio, np.uint32)), "the priorities are read only"
    return out.read(np.uint32, n), stats


def _check(sym, prio=None, plan=None):
    """colours, num_colors, rounds and widest equal the host's; twice on one plan -> (colours, stats)"""
    n = sym.num_rows
    plan = _bool_plan(sym) if plan is None else plan
    want, rounds = greedy_by_priority(sym, prio)
    for _ in range(2):                                               # (the second time from the cached verdicts)
        got, stats = _color(plan, n, prio)
        assert np.array_equal(got, want)
        assert (stats[0], stats[1], stats[3]) == summary(want, rounds)[:3]
        assert stats[2] >= 2 + 2 * stats[1]
    assert app.validate_coloring(sym, got, prio) == stats[0]
    return got, stats


def _random_prio(n, seed=0):
    return io.coloring_priorities(np.zeros(n, np.uint32), "random", seed)


@pytest.mark.parametrize("name", NAMES)
def test_drivers(gpu, name):
    raw, m, sym = graph(name)
    gc = _driver(raw)
    n, nr = m.num_rows, raw.num_rows
    assert np.array_equal(gc.degrees_, np.diff(sym.adj_indptr.astype(np.int64)))
    ip = sym.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(ip))
    for order in ORDERS:
        prio, want, rounds = reference(name, order)
        got = gc.run(order)
        assert got.dtype == np.uint32 and got.shape == (n,) and gc.n_real_ == nr and gc.colors_ is got
        assert np.array_equal(got, want)
        assert (prio is None and gc.priorities_ is None) or np.array_equal(gc.priorities_, prio)
        assert (gc.num_colors_, gc.rounds_, gc.widest_) == summary(want, rounds)[:3]
        if name in RECORDS:
            assert (gc.num_colors_, gc.rounds_, gc.widest_, int(got.sum())) == RECORDS[name][order]
        assert app.validate_coloring(raw, got, gc.priorities_) == gc.num_colors_
        assert not got[nr:].any() and gc.degeneracy_ is None
        if sym.nnz:
            assert gc.launches_ >= 2 + 2 * gc.rounds_
        else:                                                        # (eye_10: an empty graph, nothing is launched)
            assert (gc.num_colors_, gc.rounds_, gc.launches_, gc.widest_) == (1, 1, 0, n)
        mis = gc.independent_set()
        assert mis.dtype == bool and mis.shape == (n,) and not mis[nr:].any() and np.array_equal(mis[:nr], want[:nr] == 0)
        assert not np.any(mis[rows] & mis[sym.adj_indices]), "independent"
        covered = np.bincount(rows[mis[sym.adj_indices]], minlength=n) > 0
        assert np.all(mis[:nr] | covered[:nr]), "maximal: every other real vertex has a neighbour in it"
        assert gc.color_sizes_.shape == (gc.num_colors_,) and int(gc.color_sizes_.sum()) == nr
        assert all(gc.color_sizes_[c] == np.count_nonzero(want[:nr] == c) for c in range(gc.num_colors_))
        top = gc.independent_set(gc.num_colors_ - 1)
        assert np.array_equal(np.flatnonzero(top), np.flatnonzero(want[:nr] == gc.num_colors_ - 1)) and not gc.independent_set(gc.num_colors_).any()
    assert np.array_equal(gc.run(), reference(name, "largest_first")[1]), "the default order"


@pytest.mark.parametrize("name", NAMES)
def test_smallest_last_needs_at_most_degeneracy_plus_one_colours(gpu, name):
    raw, m, sym = graph(name)
    gc = _driver(raw)
    got = gc.run("smallest_last")
    n = m.num_rows
    assert gc.priorities_.dtype == np.uint32 and np.array_equal(np.sort(gc.priorities_), np.arange(n, dtype=np.uint32))
    want, rounds = greedy_by_priority(sym, gc.priorities_)
    assert np.array_equal(got, want)
    assert (gc.num_colors_, gc.rounds_, gc.widest_) == summary(want, rounds)[:3]
    assert gc.num_colors_ <= gc.degeneracy_ + 1
    if name in KCORE_RECORDS:
        assert gc.degeneracy_ == KCORE_RECORDS[name][0]
    else:
        assert gc.degeneracy_ == {"line_8": 1, "eye_10": 0, "many": 2}[name]
    assert app.validate_coloring(raw, got, gc.priorities_) == gc.num_colors_
    # every vertex has at most degeneracy neighbours before it in this order: the property the bound rests on
    rows = np.repeat(np.arange(n), np.diff(sym.adj_indptr.astype(np.int64)))
    p = gc.priorities_.astype(np.int64)
    assert np.bincount(rows[p[sym.adj_indices] > p[rows]], minlength=n).max() <= gc.degeneracy_
    assert gc.run("natural") is not None and gc.degeneracy_ is None and gc.priorities_ is None


@pytest.mark.parametrize("name", ["uniform_10K_10", "rmat_20K"])
@pytest.mark.parametrize("order", ["random", "largest_first"])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, name, order):
    build_cpp_driver("coloring_driver.cpp")
    raw = graph(name)[0]
    _, want, rounds = reference(name, order)
    path = str(tmp_path / (name + "_csr_float32.npz"))
    save_npz(path, raw)
    r = subprocess.run([COLORING_DRIVER, path, str(tmp_path), order, "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GraphColoring::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "cpp_color.bin"), dtype=np.uint32)
    assert np.array_equal(got, want)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    rec = RECORDS[name][order]
    for line in ("colours: %d" % rec[0], "rounds: %d" % rec[1], "widest: %d" % rec[2], "sum of colours: %d" % rec[3], "checksum: %d" % checksum):
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])


def test_cpp_driver_smallest_last(gpu, tmp_path):
    """the peeling order is not unique, so the colours are not compared: the driver checks the bound and that the colouring is proper"""
    build_cpp_driver("coloring_driver.cpp")
    raw, m, _ = graph("rmat_20K")
    path = str(tmp_path / "rmat_20K_csr_float32.npz")
    save_npz(path, raw)
    r = subprocess.run([COLORING_DRIVER, path, str(tmp_path), "smallest_last", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GraphColoring::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "cpp_color.bin"), dtype=np.uint32)
    assert app.validate_coloring(m, got) <= KCORE_RECORDS["rmat_20K"][0] + 1


@pytest.mark.parametrize("k", [2, 3, 5, 9, 10, 33, 34, 64, 65, 66, 129, 258])
def test_cliques_across_the_step_the_cut_the_masks_and_the_windows(gpu, k):
    """K_k on exactly k vertices: rows of k - 1 entries -- within one 4-entry step, across the cut (8 entries by default), the
    thread's 64-bit mask, the 64-bit masks of the wavefront's 256-colour window, that window (K_258: colours 256 and 257 are found
    by a second pass) and the 256-entry takeover step.  Every vertex waits for all before it: k rounds of one vertex."""
    a, b = _clique_edges(k, 0)
    g = _graph(k, a, b)
    plan = _bool_plan(g)
    for _ in range(2):
        got, stats = _color(plan, k)
        assert np.array_equal(got, np.arange(k, dtype=np.uint32))
        assert (stats[0], stats[1], stats[3]) == (k, k, 1)
    up = np.arange(k, dtype=np.uint32)                               # prio[i] = i: the last vertex first
    got, stats = _color(plan, k, up)
    assert np.array_equal(got, (k - 1 - np.arange(k)).astype(np.uint32))
    assert (stats[0], stats[1], stats[3]) == (k, k, 1)
    _check(g, _random_prio(k, 3), plan)
    # the same clique inside a padded matrix: the isolated vertices take colour 0 in round 1
    n = 512 if k > 66 else 256
    got, stats = _color(_bool_plan(_graph(n, a + 5, b + 5)), n)
    want = np.zeros(n, np.uint32)
    want[5:5 + k] = np.arange(k)
    assert np.array_equal(got, want) and (stats[0], stats[1], stats[3]) == (k, k, n - k + 1)


@pytest.mark.parametrize("k,holes", [(200, (70, 0, 63, 64, 199)), (600, (255, 256, 300, 511, 512, 599))])
def test_a_hole_in_a_later_mask_or_window(gpu, k, holes):
    """K_k in natural order gives vertex i colour i.  A later vertex x adjacent to all of it except vertex h finds colour h free,
    wherever h lies: in the first 64-bit mask, a later one, or (K_600) a later 256-colour window, which a pass that only reads
    colours searches; y, adjacent to all k, gets colour k.  One x per hole, not adjacent to each other."""
    a, b = _clique_edges(k, 0)
    ea, eb = [a], [b]
    for j, h in enumerate(holes):
        others = np.delete(np.arange(k), h)
        ea.append(np.full(k - 1, k + j))
        eb.append(others)
    y = k + len(holes)
    ea.append(np.full(k, y))
    eb.append(np.arange(k))
    n = y + 1
    g = _graph(n, np.concatenate(ea), np.concatenate(eb))
    got, stats = _check(g)
    assert np.array_equal(got[:k], np.arange(k, dtype=np.uint32))
    assert got[k:y].tolist() == list(holes) and got[y] == k
    # the x without vertex k - 1 shares round k with it; the other x and y share round k + 1
    assert (stats[0], stats[1], stats[3]) == (k + 1, k + 1, len(holes))


def test_mask_of_a_thread_that_finishes_a_row_of_64_entries(gpu, monkeypatch):
    """color_cut = 64, its cap: K_65's rows of 64 entries are finished by one thread, whose mask of the colours 0 .. 63 is full
    for the last vertex (colour 64); K_66's rows of 65 entries go to the wavefront.  A larger value is clamped to 64."""
    for cut in (64, 1000):
        set_knob(monkeypatch, "color_cut", cut)
        for k in (64, 65, 66):
            a, b = _clique_edges(k, 0)
            got, stats = _check(_graph(k, a, b))
            assert np.array_equal(got, np.arange(k, dtype=np.uint32)) and stats[1] == k


def test_path_longer_than_any_batch(gpu):
    """5000 vertices in a row in natural order: vertex i waits for i - 1, so 5000 rounds of one vertex -- more than a batch
    enqueues, so the gating carries the run across batches -- and the colours alternate"""
    n = 5000
    v = np.arange(n)
    g = _graph(n, v[:-1], v[1:])
    plan = _bool_plan(g)
    got, stats = _color(plan, n)
    assert np.array_equal(got, (v & 1).astype(np.uint32))
    assert (stats[0], stats[1], stats[3]) == (2, n, 1) and stats[2] >= 2 + 2 * n
    got, stats = _check(g, _random_prio(n), plan)
    assert stats[0] <= 3
    rng = np.random.default_rng(5)                                   # the same path under shuffled vertex numbers
    p = rng.permutation(n)
    _check(_graph(n, p[v[:-1]], p[v[1:]]))


def test_cycle_tree_star_bipartite_and_crown(gpu):
    # an odd cycle needs three colours
    n = 501
    v = np.arange(n)
    g = _graph(n, v, np.roll(v, -1))
    got, stats = _check(g)
    assert stats[0] == 3 and got[n - 1] == 2 and np.array_equal(got[:n - 1], (v[:n - 1] & 1).astype(np.uint32))
    _check(g, _random_prio(n, 1))
    # a complete binary tree of 2047 vertices: two colours by generation in natural order, one generation per round
    n = 2047
    child = np.arange(1, n)
    g = _graph(n, (child - 1) // 2, child)
    got, stats = _check(g)
    assert stats[0] == 2 and stats[1] == 11 and stats[3] == 1024
    _check(g, _random_prio(n, 2))
    # a star of 5000 leaves with the hub first ...
    n = 5001
    g = _graph(n, np.zeros(5000, np.int64), np.arange(1, n))
    got, stats = _check(g)
    assert got[0] == 0 and np.all(got[1:] == 1) and (stats[0], stats[1], stats[3]) == (2, 2, 5000)
    _check(g, _random_prio(n, 3))
    # ... and with the hub last: 5000 concurrent decrements of one word, which is appended once; two rounds
    g = _graph(n, np.full(5000, 5000), np.arange(5000))
    got, stats = _check(g)
    assert got[5000] == 1 and not got[:5000].any() and (stats[0], stats[1], stats[3]) == (2, 2, 5000)
    _check(g, _random_prio(n, 4))
    # complete bipartite K_{40,300}
    a, b = np.meshgrid(np.arange(40), np.arange(40, 340), indexing="ij")
    g = _graph(340, a.ravel(), b.ravel())
    got, stats = _check(g)
    assert stats[0] == 2 and stats[1] == 2
    got, stats = _check(g, _random_prio(340, 5))
    assert stats[0] == 2
    # the crown graph on 2 x 40 vertices -- a_i = 2 i is adjacent to b_j = 2 j + 1 for i != j -- in the pairing order a_0, b_0,
    # a_1, b_1, ...: first-fit gives a_i and b_i colour i, 40 colours for a bipartite graph
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    keep = i != j
    g = _graph(80, 2 * i[keep], 2 * j[keep] + 1)
    got, stats = _check(g)
    assert stats[0] == 40 and np.array_equal(got, (np.arange(80) // 2).astype(np.uint32))
    sides = np.where(np.arange(80) % 2 == 0, 2, 1).astype(np.uint32)     # one side first: two colours
    got, stats = _check(g, sides)
    assert stats[0] == 2


def test_cliques_joined_by_a_path_and_pendant_vertices(gpu):
    # K_20 on 4 .. 23, K_50 on 24 .. 73, a path 23 - 74 - ... - 85 - 24 between them, a path 86 - ... - 95 hanging off 85
    n = 256
    a1, b1 = _clique_edges(20, 4)
    a2, b2 = _clique_edges(50, 24)
    chain = np.concatenate([[23], np.arange(74, 86), [24]])
    tail = np.arange(85, 96)
    g = _graph(n, np.concatenate([a1, a2, chain[:-1], tail[:-1]]), np.concatenate([b1, b2, chain[1:], tail[1:]]))
    got, stats = _check(g)
    assert stats[0] == 50 and np.array_equal(got[4:24], np.arange(20)) and np.array_equal(got[24:74], np.arange(50))
    _check(g, _random_prio(n, 6))
    _check(g, io.coloring_priorities(np.diff(g.adj_indptr.astype(np.int64)), "largest_first", 0))
    # K_40 on 6 .. 45 with a pendant vertex on every member (and three on the first)
    n = 384
    a, b = _clique_edges(40, 6)
    g = _graph(n, np.concatenate([a, np.arange(6, 46), [6, 6, 6]]), np.concatenate([b, np.arange(100, 140), [200, 201, 202]]))
    got, stats = _check(g)
    assert stats[0] == 40 and got[100] == 1 and not got[101:140].any()
    _check(g, _random_prio(n, 7))


def test_explicit_priorities(gpu):
    raw, m, sym = graph("rmat_20K")
    n = sym.num_rows
    plan = _bool_plan(sym)
    natural = reference("rmat_20K", "natural")[1]
    for value in (0, 7, 0xFFFFFFFF):                                 # all equal: the natural order
        got, stats = _color(plan, n, np.full(n, value, np.uint32))
        assert np.array_equal(got, natural) and stats[0] == RECORDS["rmat_20K"]["natural"][0]
    # the largest words: no sign, no wrap
    rng = np.random.default_rng(8)
    big = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 0], np.uint32), size=n)
    got_big, stats_big = _check(sym, big, plan)
    # a second call with other priorities leaves nothing of the first: the same as on a fresh plan
    prio = reference("rmat_20K", "random")[0]
    got, stats = _color(plan, n, prio)
    fresh, fresh_stats = _color(_bool_plan(sym), n, prio)
    assert np.array_equal(got, fresh) and np.array_equal(got, reference("rmat_20K", "random")[1]) and stats == fresh_stats
    again, again_stats = _color(plan, n, prio)                       # a repeated call is bit-identical
    assert np.array_equal(again, got) and again_stats == stats
    back, back_stats = _color(plan, n, big)
    assert np.array_equal(back, got_big) and back_stats == stats_big
    # the driver: an array of n_real_ or of n_ words overrides `order`
    gc = _driver(raw)
    nr = raw.num_rows
    assert n > nr
    for p in (prio[:nr], prio):
        got = gc.run(order="natural", priorities=p)
        assert np.array_equal(gc.priorities_[:p.shape[0]], p) and gc.priorities_.shape == (n,) and not gc.priorities_[p.shape[0]:].any()
        assert np.array_equal(got, greedy_by_priority(sym, gc.priorities_)[0])
        assert app.validate_coloring(raw, got, p) == gc.num_colors_
    with pytest.raises(ValueError, match="priorities of shape"):
        gc.run(priorities=prio[:100])


@pytest.mark.parametrize("cut", [0, 4, 32])
@pytest.mark.parametrize("batch", [1, 2, 64])
def test_knobs_change_neither_the_colours_nor_the_rounds(gpu, monkeypatch, cut, batch):
    """rounds and widest are properties of (graph, order): neither where the wavefront takes a row over nor how many launches are
    enqueued between two read-backs of the control record changes them; the knobs are read per call"""
    _, m, sym = graph("rmat_20K")
    n = sym.num_rows
    plan = _bool_plan(sym)
    prio, want, rounds = reference("rmat_20K", "random")
    _, base = _color(plan, n, prio)
    v = np.arange(600)
    path = _graph(600, v[:-1], v[1:])
    path_plan = _bool_plan(path)
    set_knob(monkeypatch, "color_cut", cut)
    set_knob(monkeypatch, "color_batch", batch)
    got, stats = _color(plan, n, prio)
    assert np.array_equal(got, want)
    assert (stats[0], stats[1], stats[3]) == (base[0], base[1], base[3]) == RECORDS["rmat_20K"]["random"][:3]
    assert (stats[2] - 2) % (2 * batch) == 0 and stats[2] >= 2 + 2 * stats[1]
    if batch == 1:
        assert stats[2] == 2 + 2 * stats[1]                          # one pair per round, the last of which finds the empty slice
    got, stats = _color(plan, n)                                     # (no priorities: the binary search of init)
    assert np.array_equal(got, reference("rmat_20K", "natural")[1]) and (stats[0], stats[1], stats[3]) == RECORDS["rmat_20K"]["natural"][:3]
    got, stats = _color(path_plan, 600)
    assert np.array_equal(got, (v & 1).astype(np.uint32)) and (stats[0], stats[1], stats[3]) == (2, 600, 1)
    assert (stats[2] - 2) % (2 * batch) == 0


def test_grid_knob(gpu, monkeypatch):
    _, m, sym = graph("rmat_20K")
    prio, want, _ = reference("rmat_20K", "largest_first")
    plan = _bool_plan(sym)
    for per_cu in (1, 16):
        set_knob(monkeypatch, "color_grid", per_cu)
        got, stats = _color(plan, sym.num_rows, prio)
        assert np.array_equal(got, want) and (stats[0], stats[1], stats[3]) == RECORDS["rmat_20K"]["largest_first"][:3]


def test_entry_list_with_a_nonzero_first_offset(gpu):
    """the C ABI accepts a whole-matrix CSR whose indptr[0] is k != 0: the row copy's offsets then count from the caller's entry
    list while its indices start at entry k (csr_nz_base)"""
    _, m, sym = graph("uniform_10K_10")
    n, k = sym.num_rows, 77
    junk = np.full(k, n - 1, np.uint32)                              # (entries in front of row 0 that belong to no row)
    plan = capi.SpMVPlan(n, n, sym.adj_indptr + np.uint32(k), np.concatenate([junk, sym.adj_indices]),
                         np.concatenate([np.ones(k, np.float32), sym.adj_data]), 0, n, flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean" and plan.info()["nnz"] == sym.nnz
    for order in ORDERS:
        prio, want, rounds = reference("uniform_10K_10", order)
        got, stats = _color(plan, n, prio)
        assert np.array_equal(got, want) and (stats[0], stats[1], stats[3]) == RECORDS["uniform_10K_10"][order][:3]
    # hub rows through the wavefront's takeover: a star's row of 5000 entries and K_200
    a, b = _clique_edges(200, 1)
    g = _graph(5120, np.concatenate([np.zeros(5000, np.int64), a]), np.concatenate([np.arange(1, 5001), b]))
    plan = capi.SpMVPlan(5120, 5120, g.adj_indptr + np.uint32(k), np.concatenate([junk * 0, g.adj_indices]),
                         np.concatenate([np.ones(k, np.float32), g.adj_data]), 0, 5120, flags=capi.GL_PLAN_BOOLEAN)
    for prio in (None, _random_prio(5120, 9), (5120 - np.arange(5120)).astype(np.uint32)[::-1].copy()):
        _check(g, prio, plan)


def test_empty_plan_and_a_diagonal(gpu):
    n = 256
    e = _csr(n, [], [])                          # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for prio in (None, _random_prio(n)):
        for _ in range(2):
            got, stats = _color(empty, n, prio)
            assert not got.any() and stats == (1, 1, 0, n)
    # only a diagonal: the ABI ignores an entry (v, v), so nobody has a neighbour -- one colour, one round
    d = _sorted_rows(_csr(n, [3, 4, 9], [3, 4, 9]))
    plan = _bool_plan(d)
    for prio in (None, _random_prio(n), np.arange(n, dtype=np.uint32)):
        got, stats = _color(plan, n, prio)
        assert not got.any() and (stats[0], stats[1], stats[3]) == (1, 1, n)
    # a triangle 3 - 4 - 5 with a diagonal entry on 3, on 4 and on the isolated vertex 9
    a, b = np.array([3, 4, 5, 3, 4, 5, 3, 4, 9]), np.array([4, 5, 3, 5, 3, 4, 3, 4, 9])
    d = _sorted_rows(_csr(n, a, b))
    got, stats = _check(d)
    assert got[3:6].tolist() == [0, 1, 2] and (stats[0], stats[1], stats[3]) == (3, 3, n - 2)
    _check(d, np.arange(n, dtype=np.uint32))


def test_refusals(gpu):
    _, m, sym = graph("uniform_10K_10")
    n = sym.num_rows
    plan = _bool_plan(sym)
    prio, want, _ = reference("uniform_10K_10", "random")

    def still_works():
        got, stats = _color(plan, n, prio)
        assert np.array_equal(got, want) and stats[0] == RECORDS["uniform_10K_10"]["random"][0]
    still_works()
    out = capi.DeviceBuffer.from_host(np.full(n + 128, GARBAGE, np.uint32))
    dprio = capi.DeviceBuffer.from_host(prio)

    def refused(p, *needles):
        for d in (None, dprio, None):                                       # (the later times from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.color(d, out)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and "gl_color" in str(e.value), str(e.value)
            assert all(needle in str(e.value) for needle in needles), str(e.value)
            assert all(needle in capi.lib().gl_last_error().decode() for needle in needles)
        assert np.all(out.read(np.uint32, n + 128) == GARBAGE), "a refused call writes nothing"
        still_works()
    general = capi.SpMVPlan(sym.num_rows, sym.num_cols, sym.adj_indptr, sym.adj_indices, sym.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "row copy")
    refused(_bool_plan(sym, 0, n // 2), "row shard")
    refused(_bool_plan(sym, n // 2, n), "row shard")
    sh = permute_rows(sym, 77)
    assert not np.array_equal(sh.adj_indices, sym.adj_indices)
    refused(_bool_plan(sh), "io.symmetrize_simple")                         # unsorted rows (or, row by row, no longer symmetric)
    rows = np.repeat(np.arange(n), np.diff(sym.adj_indptr.astype(np.int64)))
    unsorted = sym.copy()
    unsorted.adj_indices = sym.adj_indices[np.lexsort((-sym.adj_indices.astype(np.int64), rows))]      # every row descending
    refused(_bool_plan(unsorted), "strictly ascending", "io.symmetrize_simple")
    wide = io.CSRMatrix(n, n + 128, sym.adj_data, sym.adj_indices, sym.adj_indptr)
    refused(_bool_plan(wide), "num_rows == num_cols")
    # one edge stored one way only: K_5 on 10 .. 14 in both directions, and (20, 21) without (21, 20)
    a, b = _clique_edges(5, 10)
    one_way = _sorted_rows(_csr(256, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]])))
    p1 = _bool_plan(one_way)
    for _ in range(2):
        with pytest.raises(capi.GraphLilyError) as e:
            p1.color(None, out)
        assert e.value.code == capi.GL_ERR_UNSUPPORTED and "not symmetric" in str(e.value) and "io.symmetrize_simple" in str(e.value)
    # with the edge's other copy the same graph is accepted
    both = _graph(256, np.concatenate([a, [20]]), np.concatenate([b, [21]]))
    got, _ = _color(_bool_plan(both), 256)
    assert got[10:15].tolist() == [0, 1, 2, 3, 4] and (got[20], got[21]) == (0, 1) and int(got.sum()) == 11
    with pytest.raises(capi.GraphLilyError) as e:
        plan.color(None, None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    with pytest.raises(capi.GraphLilyError) as e:
        plan.color(out, out)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    assert capi.lib().gl_color(None, None, ctypes.c_void_p(out.ptr), None) == capi.GL_ERR_INVALID_ARG
    assert np.all(out.read(np.uint32, n + 128) == GARBAGE)
    # NULL stats are accepted
    assert capi.lib().gl_color(ctypes.c_void_p(plan.handle), None, ctypes.c_void_p(out.ptr), None) == capi.GL_OK
    assert np.array_equal(out.read(np.uint32, n), reference("uniform_10K_10", "natural")[1])
    still_works()
