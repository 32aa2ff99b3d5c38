"""GPU parity of the neighbourhood-similarity kernel (gl_similarity, SpMVPlan.similarity, SpMVModule.similarity, app.Similarity,
graphlily::app::Similarity) against the host model kept in tests/test_similarity_cpu.py (similarity_model: Python sets and integer
sums, which that file checks against networkx).  The counts and the weighted sums are integers, so every comparison is
np.array_equal.  Every test runs with the default knobs and with sim_short=0, which defers every pair with a non-empty shorter row
to the wavefront-per-pair pass; every output buffer starts as garbage with guard words behind it.  This caller's contract cases
(gl_rows.h) live here."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver, set_knob
from test_kcore_cpu import _csr
from test_similarity_cpu import (GOLDEN, EXPECTED, MEASURES, NONE, SIMILARITY_DRIVER, all_pairs, deferred_model, model_result, nx_case,
                                 similarity_model, sym_of, tables_of, test_library_exports_and_binds_the_entry_point)

pytestmark = pytest.mark.gpu

G32, G64 = 0xdeadbeef, 0xdeadbeefdeadbeef
GUARD = 64
DEFAULT_SHORT = 64               # sim_short's default (gl_sim.hip)
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.fixture(autouse=True, params=[None, 0], ids=["short_and_deferred", "all_deferred"])
def cap(request, monkeypatch):
    """every test runs twice: with the default cap -- a sub-wave group answers the pairs whose shorter row has at most sim_short
    entries, the others are deferred -- and with sim_short=0, the deferred path for everything.  -> the cap in force"""
    set_knob(monkeypatch, "sim_short", request.param)
    return DEFAULT_SHORT if request.param is None else request.param


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean" or m.nnz == 0
    return plan


class Out:
    """the pairs and the two output arrays on the device: garbage with GUARD guard words behind each output"""

    def __init__(self, pairs, weighted=True):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        self.m = m = pairs.shape[0]
        self.pairs = capi.DeviceBuffer.from_host(pairs.astype(np.uint32).ravel() if m else np.zeros(2, np.uint32))
        self.common = capi.DeviceBuffer.from_host(np.full(m + GUARD, G32, np.uint32))
        self.weighted = capi.DeviceBuffer.from_host(np.full(m + GUARD, G64, np.uint64)) if weighted else None

    def read(self):
        """-> (common, weighted or None); the guard words must still be garbage"""
        m = self.m
        common = self.common.read(np.uint32, m + GUARD)
        assert np.all(common[m:] == G32), "a guard word behind common was written"
        weighted = None
        if self.weighted is not None:
            weighted = self.weighted.read(np.uint64, m + GUARD)
            assert np.all(weighted[m:] == G64), "a guard word behind weighted was written"
            weighted = weighted[:m]
        return common[:m], weighted


def _weights(values):
    return capi.DeviceBuffer.from_host(np.ascontiguousarray(values, dtype=np.uint64))


def _sim(plan, pairs, weight=None, weighted=True):
    """-> (common, weighted or None, stats)"""
    out = Out(pairs, weighted and weight is not None)
    stats = plan.similarity(out.pairs, out.common, out.weighted, None if weight is None else _weights(weight), True, out.m)
    capi.sync()
    assert len(stats) == 4 and G64 not in stats and stats[3] == 0
    return out.read() + (stats,)


def _check(csr, pairs, weight=None, plan=None, cap=None, calls=2, what=""):
    """the kernel against the model, twice (the second time from the cached scratch: identical bits) -> the last result"""
    plan = _bool_plan(csr) if plan is None else plan
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    common, weighted = similarity_model(csr, pairs, weight)
    bad = int(np.count_nonzero((pairs >= csr.num_rows).any(axis=1)))
    for _ in range(calls):
        got = _sim(plan, pairs, weight)
        assert np.array_equal(got[0], common), "%s common: first difference at pair %d" % (what, int(np.flatnonzero(got[0] != common)[0]))
        if weight is not None:
            assert np.array_equal(got[1], weighted), "%s weighted: first difference at pair %d" % (what, int(np.flatnonzero(got[1] != weighted)[0]))
        assert got[2][0] == bad, (what, got[2])
        if cap is not None and csr.nnz:
            assert got[2][1] == deferred_model(csr, pairs, cap), (what, got[2], cap)
    return got


# ------------------------------------------------------------------ row lengths
@functools.lru_cache(maxsize=None)
def _lengths_case():
    """A directed pattern (rows are sets, nothing more is asked): vertex i < 19 has a row of LENGTHS[i] columns drawn from a pool
    of 400 vertices (19 .. 418), vertex 19 + i is its twin (the same row: every entry a hit), vertex 38 + i holds the FIRST entry
    of row i alone and 57 + i the LAST (a hit at the first / the last position of the longer row), vertex 76 a row of 40 columns
    from a pool of its own (no hit at all).  -> (csr, pairs, weights): all ordered pairs among the first 19 vertices, u == v
    included, the twins, the first / last singletons from either side, and vertex 76 against everybody."""
    rng = np.random.default_rng(19)
    k, n = len(LENGTHS), 500
    rows, cols = [], []
    own = [np.sort(rng.choice(np.arange(19, 419), size=L, replace=False)) for L in LENGTHS]
    for i, c in enumerate(own):
        for v in (i, k + i):
            rows.append(np.full(c.shape[0], v))
            cols.append(c)
        if c.shape[0]:
            rows += [np.array([2 * k + i]), np.array([3 * k + i])]
            cols += [c[:1], c[-1:]]
    rows.append(np.full(40, 4 * k))
    cols.append(np.arange(440, 480))
    csr = _csr(n, np.concatenate(rows), np.concatenate(cols))
    i, j = np.divmod(np.arange(k * k), k)
    pairs = [np.stack([i, j], axis=1)]
    a = np.arange(k)
    pairs += [np.stack([a, k + a], axis=1), np.stack([2 * k + a, a], axis=1), np.stack([a, 3 * k + a], axis=1),
              np.stack([3 * k + a, k + a], axis=1), np.stack([np.full(k, 4 * k), a], axis=1), np.array([[4 * k, 4 * k]])]
    pairs = np.concatenate(pairs).astype(np.int64)
    weights = (1 << 40) + np.arange(n, dtype=np.uint64)
    for arr in (csr.adj_indptr, csr.adj_indices, csr.adj_data, pairs, weights):
        arr.setflags(write=False)
    return csr, pairs, weights


@pytest.mark.parametrize("group", [8, 16, 32, 64])
def test_row_lengths_on_every_side_of_the_group_widths(gpu, monkeypatch, cap, group):
    set_knob(monkeypatch, "sim_group", group)
    csr, pairs, weights = _lengths_case()
    got = _check(csr, pairs, weights, cap=cap, what="group %d" % group)
    k = len(LENGTHS)
    assert got[0][:k * k].reshape(k, k).diagonal().tolist() == list(LENGTHS)           # u == v: the whole row
    assert got[0][k * k:k * k + k].tolist() == list(LENGTHS)                            # twins: every entry a hit
    assert got[0][k * k + k:k * k + 3 * k].tolist() == [min(L, 1) for L in LENGTHS] * 2  # the first entry, the last entry
    assert not got[0][k * k + 4 * k:k * k + 5 * k].any() and got[0][-1] == 40             # no hit at all


@pytest.mark.parametrize("short", [32, 33, 34])
def test_both_sides_of_the_cap(gpu, monkeypatch, short):
    """rows of 33 entries: with sim_short = 32 their pairs are deferred, with 33 and 34 a group answers them"""
    set_knob(monkeypatch, "sim_short", short)
    csr, pairs, weights = _lengths_case()
    got = _check(csr, pairs, weights, cap=short)
    both = np.minimum(np.diff(csr.adj_indptr.astype(np.int64))[pairs[:, 0]], np.diff(csr.adj_indptr.astype(np.int64))[pairs[:, 1]])
    assert got[2][1] == np.count_nonzero(both > short) and np.count_nonzero(both == 33) > 0


# ------------------------------------------------------------------ pair counts
@functools.lru_cache(maxsize=None)
def _small():
    sym, deg = sym_of(nx_case("gnp_60_0.15"))
    for arr in (sym.adj_indptr, sym.adj_indices, sym.adj_data):
        arr.setflags(write=False)
    return sym, deg


@pytest.mark.parametrize("group", [8, 16, 32, 64])
def test_pair_counts_around_a_workgroup(gpu, monkeypatch, cap, group):
    set_knob(monkeypatch, "sim_group", group)
    sym, _ = _small()
    plan = _bool_plan(sym)
    rng = np.random.default_rng(group)
    weights = rng.integers(0, 1 << 62, size=60, dtype=np.uint64)
    for m in (0, 1, 256 // group - 1, 256 // group, 256 // group + 1, 1000):
        got = _check(sym, rng.integers(0, 60, size=(m, 2)), weights, plan=plan, cap=cap, what="m = %d" % m)
        assert got[2][2] == (2 if m else 0)                              # m == 0: nothing is enqueued, nothing is written


@pytest.mark.parametrize("m", [63, 64, 65, 129])
@pytest.mark.parametrize("short", [8, 0])
def test_chunk_boundary(gpu, monkeypatch, m, short):
    """the chunk length lowered to 64: the list and its two tails are reused chunk after chunk, some deferred pairs in each"""
    set_knob(monkeypatch, "sim_chunk", 64)
    set_knob(monkeypatch, "sim_short", short)
    sym, deg = _small()
    rng = np.random.default_rng(m)
    pairs = rng.integers(0, 60, size=(m, 2))
    for lo in range(0, m - 63, 64):                                     # every full chunk: some pairs deferred, with the cap 8 not all
        assert 0 < deferred_model(sym, pairs[lo:lo + 64], short) < (65 if short == 0 else 64)
    got = _check(sym, pairs, np.arange(60) + (1 << 50), cap=short)
    assert got[2][2] == 2 * ((m + 63) // 64)


# ------------------------------------------------------------------ hubs
@functools.lru_cache(maxsize=None)
def _hubs():
    """two centres (0 and 1) that share 5000 leaves (2 .. 5001) and have 100 private leaves each; vertex 5202 is isolated"""
    shared, p0, p1 = np.arange(2, 5002), np.arange(5002, 5102), np.arange(5102, 5202)
    rows = np.concatenate([np.zeros(5100, np.int64), np.ones(5100, np.int64)])
    cols = np.concatenate([shared, p0, shared, p1])
    sym, deg = io.symmetrize_simple(_csr(5203, rows, cols))
    return sym, deg


def test_hubs(gpu, cap):
    sym, deg = _hubs()
    assert deg[0] == deg[1] == 5100 and deg[2] == 2 and deg[5002] == 1 and deg[5202] == 0
    pairs = [[0, 1], [1, 0], [0, 0], [0, 2], [5001, 1], [0, 5002], [5102, 0], [2, 3], [2, 5001], [5002, 5003], [5002, 5102], [2, 5002],
             [0, 5202], [5202, 1], [5202, 5202]]
    got = _check(sym, pairs, (1 << 40) + np.arange(5203), cap=cap)
    assert got[0].tolist() == [5000, 5000, 5100, 0, 0, 0, 0, 2, 2, 1, 0, 1, 0, 0, 0]
    assert got[2][1] == (3 if cap else 12)                              # the centre pairs; with sim_short=0 all but the isolated vertex's


# ------------------------------------------------------------------ weighted sums
def test_weighted_sums_are_64_bit_and_wrap(gpu, cap):
    sym, _ = _small()
    pairs = all_pairs(60)
    got = _check(sym, pairs, (1 << 40) + np.arange(60), cap=cap)
    assert int(got[1].max()) > 1 << 41                                   # more than 32 bits, more than one term
    # two common neighbours of weight 2^63 each: the documented wrap to 0
    square = io.symmetrize_simple(_csr(6, [0, 0, 1, 1, 0], [2, 3, 2, 3, 4]))[0]
    w = np.array([5, 7, 1 << 63, 1 << 63, 11, 13], dtype=np.uint64)
    got = _check(square, [[0, 1], [2, 3], [0, 4], [1, 1]], w)
    assert got[0].tolist() == [2, 2, 0, 2] and got[1].tolist() == [0, 12, 0, 0]


def test_weight_table_without_weighted_output(gpu):
    sym, _ = _small()
    pairs = all_pairs(60)[::5]
    out = Out(pairs, weighted=False)
    stats = _bool_plan(sym).similarity(out.pairs, out.common, None, _weights(np.arange(60)), True)
    assert np.array_equal(out.read()[0], similarity_model(sym, pairs)[0]) and stats[0] == 0


def test_order_of_a_pair_and_duplicates(gpu, cap):
    csr, pairs, weights = _lengths_case()
    both = np.concatenate([pairs, pairs[:, ::-1], pairs[:40], pairs[:40]])
    got = _check(csr, both, weights, cap=cap)
    m = pairs.shape[0]
    assert np.array_equal(got[0][:m], got[0][m:2 * m]) and np.array_equal(got[1][:m], got[1][m:2 * m])
    assert np.array_equal(got[0][2 * m:2 * m + 40], got[0][2 * m + 40:]) and np.array_equal(got[1][:40], got[1][2 * m + 40:])


# ------------------------------------------------------------------ pairs out of range
def test_pairs_out_of_range(gpu, cap):
    sym, _ = _small()
    pairs = all_pairs(60)[::9].copy()
    want = similarity_model(sym, pairs)[0]
    pairs[3] = (60, 4)
    pairs[4] = (5, 0xFFFFFFFF)
    pairs[100] = (0xFFFFFFFF, 60)
    pairs[-1] = (59, 60)
    got = _check(sym, pairs, (1 << 40) + np.arange(60), cap=cap)
    bad = np.zeros(pairs.shape[0], bool)
    bad[[3, 4, 100, -1]] = True
    assert np.all(got[0][bad] == NONE) and not got[1][bad].any() and got[2][0] == 4
    assert np.array_equal(got[0][~bad], want[~bad])                       # the neighbouring pairs are untouched


# ------------------------------------------------------------------ agreement with an existing kernel
@pytest.mark.parametrize("name", ["gnp_200_0.05", "gnp_40_0.6"])
def test_every_entry_equals_the_support_of_gl_truss(gpu, cap, name):
    sym, deg = sym_of(nx_case(name))
    plan = _bool_plan(sym)
    nnz = sym.nnz
    truss = capi.DeviceBuffer.from_host(np.full(nnz, G32, np.uint32))
    support = capi.DeviceBuffer.from_host(np.full(nnz, G32, np.uint32))
    plan.truss(truss, support)
    capi.sync()
    rows = np.repeat(np.arange(sym.num_rows, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
    pairs = np.stack([rows, sym.adj_indices.astype(np.int64)], axis=1)      # every stored entry (v, u)
    got = _sim(plan, pairs)
    want = support.read(np.uint32, nnz)
    assert np.array_equal(got[0], want) and want.any(), "first difference at entry %d" % int(np.flatnonzero(got[0] != want)[0])


# ------------------------------------------------------------------ a directed pattern
def test_directed_pattern_gives_common_predecessors(gpu, cap):
    import networkx as nx
    G = nx.gnp_random_graph(50, 0.12, seed=5, directed=True)
    e = np.array(list(G.edges()), dtype=np.int64)
    cin, cout, symmetric = io.simple_pattern(_csr(50, e[:, 1], e[:, 0]))      # an entry A[v, u] is an edge u -> v
    assert not symmetric
    pairs = all_pairs(50)
    pred = _check(cin, pairs, cap=cap)[0]
    succ = _check(cout, pairs, cap=cap)[0]
    assert pred.tolist() == [len(set(G.predecessors(u)) & set(G.predecessors(v))) for u, v in pairs.tolist()]
    assert succ.tolist() == [len(set(G.successors(u)) & set(G.successors(v))) for u, v in pairs.tolist()]
    assert not np.array_equal(pred, succ)


# ------------------------------------------------------------------ a plan without entries
@pytest.mark.parametrize("n", [1, 5, 130])
def test_plan_without_entries_answers_from_one_launch(gpu, n):
    empty = _csr(n, [], [])
    plan = capi.SpMVPlan(n, n, empty.adj_indptr, empty.adj_indices, empty.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    pairs = np.array([[0, 0], [n - 1, 0], [n, 0], [0, 0xFFFFFFFF]] + [[i % n, (3 * i) % n] for i in range(300)])
    got = _check(empty, pairs, np.arange(n) + 9, plan=plan)
    assert got[2] == (2, 0, 1, 0) and got[0].tolist() == [0, 0, NONE, NONE] + [0] * 300 and not got[1].any()


# ------------------------------------------------------------------ the contract
def test_refusals_and_invalid_arguments(gpu):
    sym, _ = _small()
    n = sym.num_rows
    plan = _bool_plan(sym)
    pairs = all_pairs(n)[::11]
    weights = _weights(np.arange(n) + 1)
    out = Out(pairs)

    def untouched():
        common, weighted = out.read()
        assert np.all(common == G32) and np.all(weighted == G64), "a refused call writes nothing"
        _check(sym, pairs, np.arange(n) + 1, plan=plan)

    def refused(p, *needles):
        for _ in range(2):                                              # (the second time through the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.similarity(out.pairs, out.common, out.weighted, weights, True, out.m)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and "gl_similarity" in str(e.value), str(e.value)
            for needle in needles:
                assert needle in str(e.value), str(e.value)
        untouched()

    general = capi.SpMVPlan(n, n, sym.adj_indptr, sym.adj_indices, sym.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "the plan keeps no row copy")
    refused(_bool_plan(sym, 0, n // 2), "row shard")
    refused(_bool_plan(io.CSRMatrix(n, n + 128, sym.adj_data, sym.adj_indices, sym.adj_indptr)), "num_rows == num_cols")
    ip = sym.adj_indptr.astype(np.int64)
    v = int(np.flatnonzero(np.diff(ip) >= 3)[0])
    unsorted = sym.adj_indices.copy()
    unsorted[ip[v]:ip[v + 1]] = unsorted[ip[v]:ip[v + 1]][::-1]
    refused(_bool_plan(io.CSRMatrix(n, n, sym.adj_data, unsorted, sym.adj_indptr)), "strictly ascending sets", "io.symmetrize_simple",
            "io.simple_pattern")
    twice = sym.adj_indices.copy()
    twice[ip[v] + 1] = twice[ip[v]]
    refused(_bool_plan(io.CSRMatrix(n, n, sym.adj_data, twice, sym.adj_indptr)), "strictly ascending sets")
    zeroed = sym.adj_data.copy()
    zeroed[ip[v]] = 0.0                                                  # stored as column 0xffffffff in the row copy
    refused(_bool_plan(io.CSRMatrix(n, n, zeroed, sym.adj_indices, sym.adj_indptr)), "strictly ascending sets")

    def invalid(needle, *args):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.similarity(*args)
        assert e.value.code == capi.GL_ERR_INVALID_ARG and needle in str(e.value) and "gl_similarity" in str(e.value), (needle, str(e.value))

    invalid("NULL d_pairs or d_common", None, out.common, None, None, True, out.m)
    invalid("NULL d_pairs or d_common", out.pairs, None, None, None, True, out.m)
    invalid("d_weighted without d_vertex_weight", out.pairs, out.common, out.weighted, None, True, out.m)
    invalid("at most 2^32 - 1", out.pairs, out.common, out.weighted, weights, True, 1 << 32)
    invalid("overlap", out.pairs, out.pairs, None, None, True, out.m)
    invalid("overlap", out.pairs, out.common, out.pairs, weights, True, out.m)
    invalid("overlap", out.pairs, out.common, out.common, weights, True, 8)
    inside = capi.DeviceBuffer(4 * 8, ptr=out.weighted.ptr + 8 * 7, keepalive=out.weighted)      # begins in the last word written
    invalid("overlap", out.pairs, inside, out.weighted, weights, True, 8)
    with pytest.raises(capi.GraphLilyError) as e:
        capi.check(capi.lib().gl_similarity(None, None, 1, None, None, None, None))
    assert e.value.code == capi.GL_ERR_INVALID_ARG and "gl_similarity" in str(e.value) and "plan != nullptr" in str(e.value)
    assert plan.similarity(None, None, None, None, True, 0) == (0, 0, 0, 0)          # m == 0: GL_OK, whatever the pointers
    untouched()


def test_header_library_and_bindings_agree(gpu):
    test_library_exports_and_binds_the_entry_point()
    assert capi.lib().gl_similarity.restype is not None


# ------------------------------------------------------------------ the module layer and the drivers
def test_module_layer(gpu, cap):
    sym, deg = _small()
    mod = M.SpMVModule(M.num_hbm_channels, 1024, 256)
    mod.set_semiring(M.LogicalSemiring)
    mod.set_mask_type(M.kNoMask)
    mod.set_up_runtime()
    mod.load_and_format_matrix(sym.copy(), True)
    mod.send_matrix_host_to_device()
    pairs = all_pairs(60)[::4]
    aa = tables_of(deg)[0]
    out = Out(pairs)
    stats = mod.similarity(out.pairs, out.common, out.weighted, _weights(aa + [0] * (mod.get_num_rows() - 60)), True, out.m)
    common, weighted = out.read()
    want = similarity_model(sym, pairs, aa)
    assert np.array_equal(common, want[0]) and np.array_equal(weighted, want[1]) and stats[:2] == (0, deferred_model(sym, pairs, cap))
    assert mod.similarity(out.pairs, out.common, None, None, False, out.m) is None      # only enqueued
    capi.sync()
    assert np.array_equal(out.read()[0], want[0])


def _driver(m):
    d = app.Similarity(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True)
    d.send_matrix_host_to_device()
    return d


def _driver_equals_model(d, raw, pairs, measures):
    got = d.run(pairs, measures)
    want = model_result(d.graph_, d.degrees_, pairs, measures)
    assert list(got) == list(measures)
    for key in measures:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    app.validate_similarity(raw, pairs, got)
    calls = max(1, sum(k in measures for k in ("adamic_adar", "resource_allocation"))) if len(pairs) and set(measures) - {"preferential_attachment"} else 0
    assert d.launches_ == 2 * calls and np.array_equal(d.pairs_, np.asarray(pairs).reshape(-1, 2))
    return got


def test_driver_on_the_golden_file(gpu, golden_dir, cap):
    path = os.path.join(golden_dir, GOLDEN)
    raw = io.load_csr_matrix_from_float_npz(path)
    want = np.load(os.path.join(golden_dir, EXPECTED))
    d = _driver(path)
    assert (d.n_, d.n_real_, d.shift_) == (128, 48, int(want["shift"]))
    got = _driver_equals_model(d, raw, want["pairs"], MEASURES)
    assert np.array_equal(got["common"], want["common"]) and np.array_equal(d.common_, want["common"])
    assert np.array_equal(d.weighted_["adamic_adar"], want["adamic_adar"]) and np.array_equal(d.weighted_["resource_allocation"], want["resource_allocation"])
    assert list(d.run(want["pairs"])) == ["common", "jaccard"] and d.launches_ == 2 and d.weighted_ == {}
    _driver_equals_model(d, raw, want["pairs"][:0], MEASURES)
    _driver_equals_model(d, raw, want["pairs"], ("resource_allocation",))
    _driver_equals_model(d, raw, want["pairs"], ("preferential_attachment",))
    edges = d.run_edges(MEASURES)
    assert d.edges_.shape == (d.graph_.nnz // 2, 2) and np.all(d.edges_[:, 0] < d.edges_[:, 1])
    assert np.array_equal(d.edges_, d.edges_[np.lexsort((d.edges_[:, 1], d.edges_[:, 0]))]) and np.array_equal(d.pairs_, d.edges_)
    app.validate_similarity(raw, d.edges_, edges)
    hub = int(np.argmax(d.degrees_))
    for source in (hub, int(d.edges_[0, 0])):
        for measure in ("jaccard", "adamic_adar", "common"):
            v, s = d.top_k(source, 5, measure)
            cand = d.two_hop_pairs([source])
            score = model_result(d.graph_, d.degrees_, cand, (measure,))[measure]
            order = np.lexsort((cand[:, 1], -score.astype(np.float64)))[:5]
            assert np.array_equal(v, cand[order, 1]) and np.array_equal(s, score[order]) and len(v) == min(5, len(cand))


def test_driver_on_a_random_graph(gpu, cap):
    sym, _ = sym_of(nx_case("gnp_200_0.05"))
    raw = sym.copy()
    d = _driver(sym.copy())
    assert d.n_ == 256 and d.n_real_ == 200
    rng = np.random.default_rng(200)
    _driver_equals_model(d, raw, rng.integers(0, 200, size=(700, 2)), MEASURES)
    got = d.run_edges(("common", "overlap", "sorensen", "cosine"))
    assert d.edges_.shape == (d.graph_.nnz // 2, 2) and got["common"].shape == (d.graph_.nnz // 2,)
    app.validate_similarity(raw, d.edges_, got)
    with pytest.raises(ValueError, match="outside the real vertices"):
        d.run([[0, 200]])


@pytest.mark.parametrize("count", [0, 300])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, golden_dir, count):
    build_cpp_driver("similarity_driver.cpp")
    path = os.path.join(golden_dir, GOLDEN)
    r = subprocess.run([SIMILARITY_DRIVER, path, str(tmp_path), str(count)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Similarity::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(path)
    if count:
        want = d.run([[(7 * i) % 48, (11 * i + 3) % 48] for i in range(count)], MEASURES)
    else:
        want = d.run_edges(MEASURES)
    read = lambda name, dtype: np.fromfile(str(tmp_path / ("cpp_%s.bin" % name)), dtype=dtype)
    assert np.array_equal(read("pairs", np.uint32), d.pairs_.astype(np.uint32).ravel())
    assert np.array_equal(read("common", np.uint32), d.common_)
    assert np.array_equal(read("aa", np.uint64), d.weighted_["adamic_adar"]) and np.array_equal(read("ra", np.uint64), d.weighted_["resource_allocation"])
    assert np.array_equal(read("aa_table", np.uint64), d.aa_) and np.array_equal(read("ra_table", np.uint64), d.ra_)
    for key in MEASURES:                                                 # the C++ scores are doubles, the integers among them exact
        got = read("score_" + key, np.uint64)
        assert np.array_equal(got, np.ascontiguousarray(want[key], dtype=np.float64).view(np.uint64)), key
    for line in ("pairs: %d" % len(d.pairs_), "shift: %d" % d.shift_, "launches: %d" % d.launches_, "deferred: %d" % d.deferred_):
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])
