"""The round-based graph kernels share their host loop and the page-locked staging words their control records are read back
into (csrc/gl_rounds.h: rounds_run, csrc/gl_common.h: staging_words), and each keeps scratch in the plan: the outcome of a call
must not depend on which of them ran before it, on the same plan or through the same staging words.  On ONE plan gl_kcore,
gl_color (natural order and one priority array), gl_truss, gl_msf, gl_match, gl_lpa, gl_louvain_move and gl_scc (the plan
declared symmetric), gl_bicc (which also uses the context's doubling words), gl_msbfs, gl_sssp_delta (one plan, whole-number
weights, a delta of 2: hundreds of buckets along the path) and gl_similarity (the staging words only) run in two different
orders, with the *_batch knobs at 1 -- many read-backs -- and at their defaults: every result array and every statistic but the
launch count equals that of the same call on a FRESH plan, and the host models'.  (The peeling order of gl_kcore is not unique:
it is validated, not compared.  The rounds of gl_scc, and the buckets, rounds and relaxations of gl_sssp_delta, follow the
hardware's schedule: they are left out as the launches are.)
The graph: a path of 300 vertices -- many rounds -- joined to a K_8 -- levels above 0, and triangles.  A symmetric pattern gives
gl_topo nothing to peel, so the same graph oriented low -> high, a DAG of 308 levels, is a second shared PAIR of plans, on which
gl_topo (weighted, topo_batch 1 and default), gl_sssp_delta and gl_scc with two plans and gl_msbfs run in two orders."""
import functools

import numpy as np
import pytest

from graphlily_amd import app, io

from helpers import set_knob
from test_bicc_cpu import RESULTS, TREE, bicc_model_of
from test_closeness_cpu import bits64, msbfs_model
from test_gpu_bicc import _bicc
from test_gpu_coloring import _color, _random_prio
from test_gpu_kcore import _bool_plan, _clique_edges, _graph, _kcore
from test_gpu_louvain import _move
from test_gpu_lpa import _lpa
from test_gpu_match import _match
from test_gpu_msbfs import _msbfs
from test_gpu_msf import _msf
from test_gpu_scc import _scc
from test_gpu_sim import _sim
from test_gpu_sssp_delta import _call as _sssp_delta, _plans as _sssp_plans, bits, dijkstra_f32
from test_gpu_topo import _topo
from test_gpu_truss import _truss
from test_louvain_cpu import move_loop
from test_lpa_cpu import greedy_colors, propagate
from test_match_cpu import greedy, pairs_of, pointer_rounds
from test_scc_cpu import scc_model
from test_similarity_cpu import similarity_model
from test_topo_cpu import topo_model

pytestmark = pytest.mark.gpu

N, PATH, K = 320, 300, 8                                    # the vertices 308 .. 319 are isolated
SWEEPS = 100
DELTA = 2.0                                                 # weights 1 .. 4: light and heavy entries, about 375 buckets along the path
MSBFS_SOURCES = [0, PATH - 1, 150, PATH + K - 1, 310]
CALLS = ["kcore", "color", "color_prio", "truss", "msf", "match", "lpa", "louvain_move", "scc", "bicc", "msbfs", "sssp_delta", "similarity"]
ORDERS = [CALLS, ["similarity", "scc", "sssp_delta", "msf", "lpa", "bicc", "truss", "match", "msbfs", "color_prio", "louvain_move", "kcore", "color"]]
DAG_CALLS = ["topo", "sssp_delta", "scc", "msbfs"]
DAG_ORDERS = [DAG_CALLS, ["msbfs", "scc", "sssp_delta", "topo"]]
KNOBS = ("kcore_batch", "color_batch", "truss_batch", "msf_batch", "match_batch", "lpa_batch", "louvain_batch", "scc_batch",
         "bicc_batch", "msbfs_batch", "sssp_delta_batch", "topo_batch")
# the index of the launch count in the stats
LAUNCHES = {"kcore": 3, "color": 2, "color_prio": 2, "truss": 3, "msf": 3, "match": 3, "lpa": 3, "louvain_move": 3, "scc": 4,
            "bicc": 4, "msbfs": 2, "sssp_delta": 4, "similarity": 2, "topo": 3}
# ... and of what else follows the hardware's schedule: gl_scc's rounds; gl_sssp_delta's buckets, rounds and relaxations
SCHEDULE = {"scc": (3,), "sssp_delta": (1, 2, 3)}


@functools.lru_cache(maxsize=None)
def _inputs():
    v = np.arange(PATH)
    a, b = _clique_edges(K, PATH)
    sym = _graph(N, np.concatenate([v[:-1], [PATH - 1], a]), np.concatenate([v[1:], [PATH], b]))
    return sym, _random_prio(N, 3), np.arange(sym.nnz, dtype=np.float32), greedy_colors(sym)


@functools.lru_cache(maxsize=None)
def _more_inputs():
    """for the newer callers -> (the graph with whole-number weights 1 .. 4, the same in both entries of an edge; 500 pairs of
    vertices; 64-bit vertex weights)"""
    sym = _inputs()[0]
    rows = np.repeat(np.arange(N), np.diff(sym.adj_indptr.astype(np.int64)))
    weighted = io.CSRMatrix(N, N, (1 + (rows + sym.adj_indices) % 4).astype(np.float32), sym.adj_indices, sym.adj_indptr)
    return weighted, np.random.default_rng(8).integers(0, N, size=(500, 2)), (1 << 40) + np.arange(N, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _dag():
    """the same graph oriented low -> high, as gl_sssp_delta's suite prepares a pair: (g_in, g_out) with the weights of
    _more_inputs() aligned with each, and the edges src -> dst in the order of g_in's entries"""
    weighted = _more_inputs()[0]
    rows = np.repeat(np.arange(N), np.diff(weighted.adj_indptr.astype(np.int64)))
    keep = weighted.adj_indices < rows                      # an entry A[v, u] is the edge u -> v
    raw = io.CSRMatrix(N, N, weighted.adj_data[keep], weighted.adj_indices[keep], np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=N))]).astype(np.uint32))
    g_in, g_out, symmetric = io.directed_weighted(raw, True, "smallest")
    assert not symmetric and g_in.nnz == g_out.nnz == weighted.nnz // 2
    dst = np.repeat(np.arange(N), np.diff(g_in.adj_indptr.astype(np.int64)))
    return g_in, g_out, g_in.adj_indices.astype(np.int64), dst


@functools.lru_cache(maxsize=None)
def _models():
    """what the host models of the four newer callers say: match (mates, (pairs, rounds, scans)) under equal weights, lpa (labels,
    (sweeps, changes, evaluations, converged)), louvain_move (labels, the stats but the launches), scc (labels, stats[:3])"""
    sym, _, _, colors = _inputs()
    mate, rounds, scans = pointer_rounds(sym)
    assert np.array_equal(mate, greedy(sym))
    lpa = propagate(sym, colors, None, SWEEPS)
    moved = move_loop(sym, None, None, colors, SWEEPS, 0)
    rows = np.repeat(np.arange(N), np.diff(sym.adj_indptr.astype(np.int64)))
    scc = scc_model(N, sym.adj_indices.astype(np.int64), rows)
    weighted, pairs, vertex_weights = _more_inputs()
    bicc = bicc_model_of(sym)
    far, reach, harmonic, hops, source_stats, levels = msbfs_model(sym, MSBFS_SOURCES)
    dist, parent, _ = dijkstra_f32(weighted, [0])
    return {"match": (mate, (len(pairs_of(mate)), rounds, scans)), "lpa": (lpa[0], tuple(lpa[1:])),
            "louvain_move": (moved[0], tuple(moved[1:])), "scc": (scc[0], tuple(scc[1:4])),
            "bicc": (tuple(bicc[k] for k in TREE + RESULTS), (bicc["blocks"], bicc["articulation"], bicc["bridges"], bicc["depth"], bicc["trees"])),
            "msbfs": ((far, reach, bits64(harmonic), hops, source_stats), tuple(levels) + (0,)),
            "sssp_delta": ((bits(dist), parent), (int(np.isfinite(dist).sum()),)),
            "similarity": (tuple(similarity_model(sym, pairs, vertex_weights)), (0, 0, 0))}


@functools.lru_cache(maxsize=None)
def _dag_models():
    """the same for the pair: topo (level, dist bits, parent), (peeled, levels, widest); sssp_delta from vertex 0; scc; msbfs over g_in"""
    g_in, g_out, src, dst = _dag()
    level, dist, parent, stats = topo_model(N, src, dst, g_in.adj_data)
    sd, sp, _ = dijkstra_f32(g_in, [0])
    scc = scc_model(N, src, dst)
    far, reach, harmonic, hops, source_stats, levels = msbfs_model(g_in, MSBFS_SOURCES)
    return {"topo": ((level, bits(dist), parent), stats), "sssp_delta": ((bits(sd), sp), (int(np.isfinite(sd).sum()),)),
            "scc": ((scc[0],), tuple(scc[1:4])), "msbfs": ((far, reach, bits64(harmonic), hops, source_stats), tuple(levels) + (0,))}


def _call(plan, call):
    """-> (the arrays to compare, the stats)"""
    sym, prio, weights, colors = _inputs()
    if call == "bicc":
        got, stats = _bicc(plan, N, sym.nnz)
        return tuple(got[k] for k in TREE + RESULTS), stats
    if call == "msbfs":
        got = _msbfs(plan, N, MSBFS_SOURCES)
        return got[:5], got[5]
    if call == "sssp_delta":
        weighted = _more_inputs()[0]
        dist, parent, stats = _sssp_delta(plan, None, weighted, weighted, [0], DELTA)
        return (dist, parent), stats
    if call == "similarity":                                # (the default cap: the rows here are short, nothing is deferred)
        common, weighted, stats = _sim(plan, _more_inputs()[1], _more_inputs()[2])
        return (common, weighted), stats
    if call == "kcore":
        core, order, stats = _kcore(plan, N)
        assert app.validate_cores(sym, core, order) == stats[0]
        return (core,), stats
    if call in ("color", "color_prio"):
        colours, stats = _color(plan, N, prio if call == "color_prio" else None)
        return (colours,), stats
    if call == "truss":
        truss, support, stats = _truss(plan, sym.nnz)
        return (truss, support), stats
    if call == "match":                                     # every weight 1, the same in both entries of an edge: the order is (lo, hi)
        mate, stats = _match(plan, sym.adj_data, N)
        return (mate,), stats
    if call == "lpa":
        label, stats = _lpa(plan, N, colors, None, SWEEPS)
        return (label,), stats
    if call == "louvain_move":
        label, stats = _move(plan, N, None, None, colors, SWEEPS, 0)
        return (label,), stats
    if call == "scc":
        label, stats = _scc(plan, None, N)
        return (label,), stats
    forest, labels, stats = _msf(plan, weights, N)
    return (forest, labels), stats


def _dag_call(pin, pout, call):
    g_in, g_out, _, _ = _dag()
    if call == "topo":
        level, order, dist, parent, stats = _topo(pin, pout, N, g_in.adj_data)
        assert np.array_equal(np.sort(order[:stats[0]]), np.flatnonzero(level != 0xffffffff)) and np.all(np.diff(level[order[:stats[0]]].astype(np.int64)) >= 0)
        return (level, dist, parent), stats
    if call == "sssp_delta":
        dist, parent, stats = _sssp_delta(pin, pout, g_in, g_out, [0], DELTA)
        return (dist, parent), stats
    if call == "scc":
        label, stats = _scc(pin, pout, N)
        return (label,), stats
    got = _msbfs(pin, N, MSBFS_SOURCES)
    return got[:5], got[5]


def _without_launches(call, stats):
    return tuple(s for i, s in enumerate(stats) if i != LAUNCHES[call] and i not in SCHEDULE.get(call, ()))


def _same_arrays(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def _fresh():
    """call -> its outcome on a plan nobody else used (under the knobs that are set now)"""
    return {call: _call(_bool_plan(_inputs()[0]), call) for call in CALLS}


@pytest.mark.parametrize("batch", [1, None])
def test_outcomes_do_not_depend_on_who_ran_before(gpu, monkeypatch, batch):
    for knob in KNOBS:
        set_knob(monkeypatch, knob, batch)
    want = _fresh()
    # the closed forms, so that the comparison below is not between two empty answers
    assert want["kcore"][1][:2] == (K - 1, 3) and want["kcore"][1][2] >= PATH - 2          # cores 0, 1 and 7; the path peels from one end
    assert want["color"][1][0] == K and want["color"][1][1] >= PATH                         # natural order: the path is one chain
    assert want["truss"][1][0] == K and want["truss"][1][4:] == (PATH + K * (K - 1) // 2, K * (K - 1) * (K - 2) // 6)
    assert want["msf"][1][:2] == (PATH + K - 1, 1 + N - PATH - K)
    models = _models()
    assert models["match"][1][0] == PATH // 2 + K // 2 and models["match"][1][1] >= PATH // 2      # (0, 1), (2, 3), ...: a pair a round
    assert models["scc"][1] == (1 + N - PATH - K, 1, N - PATH - K) and not models["scc"][0][:PATH + K].any()
    assert models["lpa"][1][0] >= 2 and models["lpa"][1][3] == 1 and np.unique(models["lpa"][0][PATH:PATH + K]).shape[0] == 1
    assert models["louvain_move"][1][0] >= 2 and models["louvain_move"][1][5] > models["louvain_move"][1][4]
    assert models["bicc"][1][0] == PATH + 1 and models["bicc"][1][2] == PATH                # 299 + 1 bridges, and the K_8: one block more
    assert models["msbfs"][0][3][0, PATH - 1] == PATH - 1 and models["sssp_delta"][1] == (PATH + K,) and models["similarity"][0][0].any()
    assert int(models["sssp_delta"][0][0].view(np.float32)[PATH - 1]) >= 100 * DELTA       # many buckets
    for call, (labels, stats) in models.items():
        labels = labels if isinstance(labels, tuple) else (labels,)
        assert _same_arrays(want[call][0], labels) and _without_launches(call, want[call][1]) == stats, call
    plan = _bool_plan(_inputs()[0])
    for order in ORDERS:
        for call in order:
            where = "%s in the order %s, batch %s" % (call, order, batch)
            arrays, stats = _call(plan, call)
            assert _same_arrays(arrays, want[call][0]), where
            assert _without_launches(call, stats) == _without_launches(call, want[call][1]), where
            if call == "kcore":
                assert stats[3] >= 1 + 3 * stats[2], where
            if call in ("color", "color_prio"):
                assert (stats[2] - 2) % (2 * (batch or 64)) == 0 and stats[2] >= 2 + 2 * stats[1], where
                if batch == 1:
                    assert stats[2] == 2 + 2 * stats[1], where


@pytest.mark.parametrize("batch", [1, None])
def test_outcomes_on_the_dag_do_not_depend_on_who_ran_before(gpu, monkeypatch, batch):
    """the pair p_in / p_out of the path and the K_8 oriented low -> high: gl_topo, gl_sssp_delta and gl_scc with two plans, and
    gl_msbfs over p_in, on ONE pair in two orders against the same calls on fresh pairs and the host models"""
    for knob in KNOBS:
        set_knob(monkeypatch, knob, batch)
    g_in, g_out, _, _ = _dag()
    pair = lambda: _sssp_plans(g_in)[2:]
    want = {call: _dag_call(*pair(), call) for call in DAG_CALLS}
    models = _dag_models()
    # the closed forms: 308 levels, one vertex each but the first, which has the 12 vertices without an edge too; nobody is on a cycle
    assert models["topo"][1] == (N, PATH + K, 1 + N - PATH - K) and np.array_equal(models["topo"][0][0][:PATH + K], np.arange(PATH + K))
    assert models["scc"][1][0] == N and models["sssp_delta"][1] == (PATH + K,) and models["msbfs"][0][3][0, PATH + K - 1] == PATH + 1
    for call, (arrays, stats) in models.items():
        assert _same_arrays(want[call][0], arrays) and _without_launches(call, want[call][1]) == stats, call
    pin, pout = pair()
    for order in DAG_ORDERS:
        for call in order:
            where = "%s in the order %s, batch %s" % (call, order, batch)
            arrays, stats = _dag_call(pin, pout, call)
            assert _same_arrays(arrays, want[call][0]), where
            assert _without_launches(call, stats) == _without_launches(call, want[call][1]), where
