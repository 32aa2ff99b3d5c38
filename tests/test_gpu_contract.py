"""GPU parity of graph contraction (gl_contract_symbolic / gl_contract_numeric, SpMVPlan.contract_*, SpMVModule.contract,
app.QuotientGraph, Louvain.run(aggregate="device")) against io.aggregate_communities -- for a directed pattern against the key
statement app.validate_quotient uses, which tests/test_contract_cpu.py checks against condensation().  Every comparison is
np.array_equal.  Every test runs with the default paths, with contract_wave=0 (no wavefront path) and with contract_lds=0 (every
group in a slab); the boundary cases also shrink the tables to 64 and 256 slots.  Outputs start as garbage with guard words
behind them, and every check is made twice: the second call runs from the cached scratch.  This caller's refusals live here;
tests/test_gpu_rows.py calls it before and behind every other asker of the plan's cached verdicts, and
test_walk_stars_in_one_group below is its part of tests/test_gpu_walk.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_contract_cpu import QUOTIENT_DRIVER, directed_graph, smallest_member
from test_gpu_louvain import _driver as louvain_driver
from test_gpu_spgemm import G32, GUARD, _bins, _plan, random_pair
from test_gpu_walk import N as STAR_N, _star_edges, _stars
from test_kcore_cpu import _csr as _csr_as_given
from test_louvain_cpu import driver_graph
from test_spgemm_cpu import GOLDEN
from test_tc_cpu import _csr

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "no_wave": {"contract_wave": 0}, "all_in_slabs": {"contract_lds": 0}}
WAVE_SLOTS, LDS_SLOTS = 64, 256


@pytest.fixture(autouse=True, params=sorted(MODES))
def mode(request, monkeypatch):
    for key, value in MODES[request.param].items():
        set_knob(monkeypatch, key, value)
    return request.param


def _small_tables(monkeypatch):
    set_knob(monkeypatch, "contract_wave_slots", WAVE_SLOTS)
    set_knob(monkeypatch, "contract_lds_slots", LDS_SLOTS)
    return WAVE_SLOTS, LDS_SLOTS


def _driver(cls, m, **how):
    d = cls(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True, **how)
    d.send_matrix_host_to_device()
    return d


def _buf(arr):
    return None if arr is None else capi.DeviceBuffer.from_host(np.ascontiguousarray(arr, np.uint32))


def _contract(plan, nv, labels, weights=None, vweights=None):
    """-> (C, weights, tot, part, symbolic stats, numeric stats); the guard words behind every output must still be garbage"""
    part, indptr = _buf(np.full(nv + GUARD, G32)), _buf(np.full(nv + 1 + GUARD, G32))
    sym = plan.contract_symbolic(nv, _buf(labels), part, indptr)
    k, nnz = sym[:2]
    pt, ip = part.read(np.uint32, nv + GUARD), indptr.read(np.uint32, nv + 1 + GUARD)
    assert np.all(pt[nv:] == G32) and np.all(ip[k + 1:] == G32), "a guard word behind d_part or d_c_indptr was written"
    assert ip[0] == 0 and ip[k] == nnz
    idx, w, tot = (_buf(np.full(size + GUARD, G32)) for size in (nnz, nnz, k))
    num = plan.contract_numeric(nv, part, k, indptr, idx, w, tot, _buf(weights), _buf(vweights), stats=True)
    i, v, t = idx.read(np.uint32, nnz + GUARD), w.read(np.uint32, nnz + GUARD), tot.read(np.uint32, k + GUARD)
    assert np.all(i[nnz:] == G32) and np.all(v[nnz:] == G32) and np.all(t[k:] == G32), "a guard word behind C or tot was written"
    return io.CSRMatrix(k, k, np.ones(nnz, np.float32), i[:nnz], ip[:k + 1]), v[:nnz], t[:k], pt[:nv], sym, num


def _check(graph, labels, mode, weights=None, vweights=None, tables=(512, 8192), directed=False, plan=None, what=""):
    """`graph`: what the plan holds; the first len(labels) vertices are labelled"""
    nv = len(labels)
    head = graph if nv == graph.num_rows else io.CSRMatrix(nv, nv, graph.adj_data, graph.adj_indices, graph.adj_indptr[:nv + 1])
    want = app._quotient_of(head, labels, weights, vweights) if directed else io.aggregate_communities(head, weights, vweights, labels)
    plan = plan or _plan(graph)
    bounds = np.bincount(want[3], np.diff(head.adj_indptr.astype(np.int64)), want[0].num_rows).astype(np.int64)
    for call in range(2):
        c, w, tot, part, sym, num = _contract(plan, nv, labels, weights, vweights)
        for got, ref in zip((c.adj_indptr, c.adj_indices, w, tot, part), (want[0].adj_indptr, want[0].adj_indices) + tuple(want[1:])):
            assert np.array_equal(got, ref), (what, call)
        head_stats = (want[0].num_rows, want[0].nnz, graph.nnz)
        assert sym == head_stats + _bins(bounds, mode, *tables) + (0,), (what, call)
        assert num == head_stats + _bins(np.diff(want[0].adj_indptr.astype(np.int64)), mode, *tables) + (0,), (what, call)
    return c, w, tot, part


def _symmetric(n, rows, cols):
    key = np.unique(np.concatenate([rows * n + cols, cols * n + rows]))
    return _csr(n, key // n, key % n)


@functools.lru_cache(maxsize=None)
def group_case(kind, c):
    """-> (symmetric graph, labels, entry weights): group 0 = the first m vertices, every other vertex a group of its own, and
    group 0 meets c of them -- `one`: m = 1, a single long row; `many`: 65 (c <= 64) or 257 members of about 1 - 3 entries each;
    `chain`: as one, the neighbours' ranks all multiples of 256, which one slot of every table serves; `inside`: as many, plus as
    many entries again between the members, which are dropped."""
    rng = np.random.default_rng(c)
    m = 1 if kind in ("one", "chain") else 65 if c <= 64 else 257
    n = m + 256 * (c + 1) if kind == "chain" else m + 1024
    nb = m - 1 + 256 * np.arange(1, c + 1) if kind == "chain" else np.sort(rng.choice(np.arange(m, n), size=c, replace=False))
    per = np.arange(max(m, c)) if m > 1 else np.arange(c)
    rows, cols = per % m, nb[per % c]                               # every member has an entry, every neighbour is met
    if m > 1:
        extra = rng.integers(0, m, size=m), nb[rng.integers(0, c, size=m)]
        rows, cols = np.concatenate([rows, extra[0]]), np.concatenate([cols, extra[1]])
    if kind == "inside":
        a, b = rng.integers(0, m, size=rows.size), rng.integers(0, m, size=rows.size)
        rows, cols = np.concatenate([rows, a[a != b]]), np.concatenate([cols, b[a != b]])
    g = _symmetric(n, rows, cols)
    labels = np.concatenate([np.zeros(m, np.uint32), np.arange(m, n, dtype=np.uint32)])
    return g, labels, rng.integers(1, 4, g.nnz).astype(np.uint32)


@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("kind", ["one", "many", "chain", "inside"])
def test_one_group_at_every_table_boundary(gpu, mode, monkeypatch, kind, c):
    tables = _small_tables(monkeypatch)
    g, labels, weights = group_case(kind, c)
    got = _check(g, labels, mode, weights, tables=tables, what="%s c=%d" % (kind, c))[0]
    assert got.adj_indptr[1] == c


@functools.lru_cache(maxsize=None)
def contract_stars(members=18, drop=None):
    """tests/test_gpu_walk.py's stars -> (symmetric graph, labels, entry weights): group 0 = the 18 hubs and, for 65 and 129
    members, the first 47 and 111 leaves (those of the smallest stars) with them; every other vertex a group of its own.  The
    weights 1 .. 3 depend on the entry's two vertices only.  `drop`: without every hub's last (first) entry and its mirror."""
    hub, leaf, kept = _star_edges(drop)
    g = _symmetric(STAR_N, hub[kept], leaf[kept])
    labels = np.arange(STAR_N, dtype=np.uint32)
    labels[_stars()[3]] = 0
    labels[leaf[:members - 18]] = 0
    rows = np.repeat(np.arange(STAR_N), np.diff(g.adj_indptr.astype(np.int64)))
    return g, labels, (1 + (rows + g.adj_indices) % 3).astype(np.uint32)


@pytest.mark.parametrize("members", [18, 65, 129])
def test_walk_stars_in_one_group(gpu, mode, members):
    """18 long member rows of every boundary length -- 0, 1, 3 .. 545 entries -- in ONE 64-member window of contract_stream, where
    group_case's members have one to three entries or are alone; with 65 and 129 members the window scan crosses 64 and 128, the
    long rows in the first window and one-entry rows behind them.  The product row holds every leaf outside the group: 2519
    distinct neighbours with 18 members.  tot comes from the row sums (no vertex weights are given): a thread for a row of at most
    16 entries, rows_walk_takeover for the longer ones.  tests/test_contract_cpu.py shows that C and tot change when the last or
    the first entry of every hub row is lost."""
    g, labels, weights = contract_stars(members)
    c, w, tot, part = _check(g, labels, mode, weights, what="%d members" % members)
    assert c.adj_indptr[1] == 2519 - (members - 18) and not part[_stars()[3]].any() and np.count_nonzero(part == 0) == members
    assert tot[0] == weights[np.repeat(labels, np.diff(g.adj_indptr.astype(np.int64))) == 0].sum()


@pytest.mark.parametrize("p", [65, 257, 1200])
def test_many_entries_into_one_slot(gpu, mode, monkeypatch, p):
    tables = _small_tables(monkeypatch)
    g = _symmetric(p + 1, np.arange(p), np.full(p, p))
    labels = np.concatenate([np.zeros(p, np.uint32), [p]]).astype(np.uint32)
    weights = np.random.default_rng(p).integers(1, 1001, g.nnz).astype(np.uint32)
    c, w, _, _ = _check(g, labels, mode, weights, tables=tables, what="p=%d" % p)
    assert c.nnz == 2 and w[0] == weights[:p].sum()


def test_a_sum_that_crosses_32_bits_is_saturated_and_counted(gpu, mode):
    g = _symmetric(4, np.arange(3), np.full(3, 3))
    labels, weights = np.array([0, 0, 0, 3], np.uint32), np.full(g.nnz, 1 << 31, np.uint32)
    c, w, tot, part, sym, num = _contract(_plan(g), 4, labels, weights)
    assert sym[:2] == (2, 2) and num[5] == 4 and w.tolist() == [0xffffffff] * 2 and tot.tolist() == [0xffffffff] * 2      # C's two words and tot's two
    d = _driver(app.QuotientGraph, g)
    with pytest.raises(ValueError, match="do not fit 32 bits"):
        d.run(labels, weights)
    assert d.run(labels)[1].tolist() == [3, 3] and d.inside_weight_ == 0 and d.num_groups_ == 2


@functools.lru_cache(maxsize=None)
def label_graph():
    """300 vertices, about 1500 edges, a diagonal entry in every seventh row; then three triangles: vertices 300 .. 302 and 306 ..
    308 joined to the rest, 303 .. 305 to nobody"""
    rng = np.random.default_rng(5)
    n = 309
    tri = [(a + i, a + (i + 1) % 3) for a in (300, 303, 306) for i in range(3)]
    rows = np.concatenate([rng.integers(0, 300, 1500), [t[0] for t in tri], [300, 307]])
    cols = np.concatenate([rng.integers(0, 300, 1500), [t[1] for t in tri], [5, 9]])
    g = _symmetric(n, np.concatenate([rows, np.arange(0, 300, 7)]), np.concatenate([cols, np.arange(0, 300, 7)]))
    return g, rng.integers(1, 100, g.nnz).astype(np.uint32)


@pytest.mark.parametrize("how", ["gaps", "singletons", "one_group", "lonely_group", "padding_rows", "unit_weights", "vertex_weights"])
def test_labels(gpu, mode, how):
    g, weights = label_graph()
    n = g.num_rows
    v = np.arange(n, dtype=np.uint32)
    if how == "gaps":
        c, _, _, part = _check(g, v // 7 * 7, mode, weights, what=how)
        assert c.num_rows == 45 and part[7] == 1
    elif how == "singletons":
        c = _check(g, v, mode, what=how)[0]
        off = np.repeat(v, np.diff(g.adj_indptr.astype(np.int64))) != g.adj_indices
        assert np.array_equal(c.adj_indices, g.adj_indices[off]) and c.nnz == g.nnz - 43
    elif how == "one_group":
        c, _, tot, _ = _check(g, np.zeros(n, np.uint32), mode, weights, what=how)
        assert c.num_rows == 1 and c.nnz == 0 and tot.shape == (1,)
    elif how == "lonely_group":
        c = _check(g, np.where(v >= 300, v // 3 * 3, 0).astype(np.uint32), mode, weights, what=how)[0]
        assert np.diff(c.adj_indptr.astype(np.int64)).tolist() == [2, 1, 0, 1]
    elif how == "padding_rows":
        padded = io.CSRMatrix(n + 75, n + 75, g.adj_data, g.adj_indices, np.concatenate([g.adj_indptr, np.full(75, g.nnz, np.uint32)]))
        _check(padded, v // 5 * 5, mode, weights, what=how)
    elif how == "unit_weights":
        assert all(np.array_equal(a, b) for a, b in zip(_check(g, v // 7 * 7, mode)[1:], _check(g, v // 7 * 7, mode, np.ones(g.nnz, np.uint32))[1:]))
    else:
        derived = io.aggregate_communities(g, weights, None, v)[2]
        assert np.array_equal(_check(g, v // 7 * 7, mode, weights, derived)[2], _check(g, v // 7 * 7, mode, weights)[2])
        _check(g, v // 7 * 7, mode, weights, derived + np.random.default_rng(1).integers(0, 50, n).astype(np.uint32), what=how)


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("labelling", ["blocks_of_7", "random_40", "smallest_member"])
def test_random_graph(gpu, mode, labelling, directed):
    raw = random_pair()[0]
    g = io.simple_pattern(raw)[0] if directed else io.symmetrize_simple(raw)[0]
    n = g.num_rows
    rng = np.random.default_rng(40)
    labels = {"blocks_of_7": np.arange(n) // 7, "random_40": rng.integers(0, 40, n), "smallest_member": smallest_member(rng.integers(0, 25, n))}[labelling]
    weights = rng.integers(1, 1000, g.nnz).astype(np.uint32)
    result = _check(g, labels.astype(np.uint32), mode, weights, directed=directed, what=labelling)
    assert app.validate_quotient(raw, labels, result, directed=directed, weights=weights) == result[0].num_rows


def test_refusals_and_the_empty_plan(gpu):
    g, _ = label_graph()
    n = g.num_rows
    labels, out = _buf(np.zeros(n)), _buf(np.full(2 * n + 2, G32))
    shuffled = _csr_as_given(n, [3, 3, 3], [9, 4, 7])
    for bad, message in ((_plan(g, flags=0), "keeps no row copy"), (_plan(g, 0, 128), "row shard"), (_plan(shuffled), "strictly ascending"),
                         (_plan(g), "not empty")):
        with pytest.raises(capi.GraphLilyError, match=message) as err:
            bad.contract_symbolic(n - 20 if message == "not empty" else n, labels, out, out)
        assert err.value.code == capi.GL_ERR_UNSUPPORTED
    plan = _plan(g)
    for nv, lab in ((n + 1, labels), (n, _buf(np.full(n, n))), (n - 9, _buf(np.full(n, n - 9)))):
        with pytest.raises(capi.GraphLilyError) as err:
            plan.contract_symbolic(nv, lab, out, out)
        assert err.value.code == capi.GL_ERR_INVALID_ARG
    with pytest.raises(capi.GraphLilyError, match="last gl_contract_symbolic") as err:       # (the refused call left no grouping)
        plan.contract_numeric(n, out, 1, out, out)
    assert err.value.code == capi.GL_ERR_INVALID_ARG
    empty = io.CSRMatrix(n, n, np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(n + 1, np.uint32))
    v = np.arange(n, dtype=np.uint32)
    c, _, tot, part = _check(empty, v // 4 * 4, "default", None, v + 1)
    assert c.nnz == 0 and not c.adj_indptr.any() and tot[0] == 1 + 2 + 3 + 4 and part[4] == 1


def test_louvain_aggregates_on_the_device(gpu):
    for name in ("planted", "rmat"):
        d = louvain_driver(driver_graph(name)[0])
        host = d.run(aggregate="host").copy()
        want = {f: getattr(d, f) for f in ("levels_", "level_sizes_", "level_colors_", "level_sweeps_", "level_moves_", "level_q_", "dendrogram_")}
        assert np.array_equal(d.run(aggregate="device"), host) and d.levels_ >= 1 and sorted(d.timings_) == ["aggregate", "color", "move", "plan"]
        for f, ref in want.items():
            got = getattr(d, f)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and len(got) == len(ref) if f == "dendrogram_" else np.array_equal(got, ref), f


def test_quotient_of_the_strong_components_is_the_condensation(gpu):
    raw = directed_graph()
    scc, q = _driver(app.StronglyConnectedComponents, raw), _driver(app.QuotientGraph, raw)
    labels = scc.run()[:scc.n_real_]
    dag, rank = scc.condensation()
    c, w, tot, part = q.run(labels)
    assert q.directed_ and np.array_equal(c.adj_indptr, dag.adj_indptr) and np.array_equal(c.adj_indices, dag.adj_indices)
    assert np.array_equal(part, rank[labels]) and q.num_groups_ == scc.num_components_ > 1 and sum(q.paths_) == np.count_nonzero(np.diff(c.adj_indptr))
    assert int(w.sum()) + q.inside_weight_ == q.graph_.nnz and app.validate_quotient(raw, labels, (c, w, tot, part)) == q.num_groups_


def test_cpp_driver_on_the_golden_file(gpu, golden_dir, tmp_path):
    path = os.path.join(golden_dir, GOLDEN)
    r = subprocess.run([QUOTIENT_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "QuotientGraph OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for directed in (False, True):
        q = _driver(app.QuotientGraph, path, directed=directed)
        labels = (np.arange(q.n_real_) // 5 * 5).astype(np.uint32)                # (the driver's labelling)
        c, w, tot, part = q.run(labels)
        want = {"indptr": c.adj_indptr, "indices": c.adj_indices, "weights": w, "tot": tot, "part": part}
        for field, ref in want.items():
            got = np.fromfile(os.path.join(str(tmp_path), "cpp_%s_%s.bin" % ("directed" if directed else "undirected", field)), dtype=np.uint32)
            assert ref.size > 1 and np.array_equal(got, ref), (directed, field)
