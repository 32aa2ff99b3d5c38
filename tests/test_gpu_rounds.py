"""The round-based graph kernels share their host loop and the page-locked staging words their control records are read back
into (csrc/gl_rounds.h: rounds_run, csrc/gl_common.h: staging_words), and each keeps scratch in the plan: the outcome of a call
must not depend on which of them ran before it, on the same plan or through the same staging words.  On ONE plan gl_kcore,
gl_color (natural order and one priority array), gl_truss, gl_msf, gl_match, gl_lpa, gl_louvain_move and gl_scc (the plan
declared symmetric) run in two different orders, with the eight *_batch knobs at 1 -- many read-backs -- and at their defaults:
every result array and every statistic but the launch count equals that of the same call on a FRESH plan, and the host models'.
(The peeling order of gl_kcore is not unique: it is validated, not compared.  The rounds of gl_scc follow the hardware's
schedule: they are left out as the launches are.)
The graph: a path of 300 vertices -- many rounds -- joined to a K_8 -- levels above 0, and triangles."""
import functools

import numpy as np
import pytest

from graphlily_amd import app

from helpers import set_knob
from test_gpu_coloring import _color, _random_prio
from test_gpu_kcore import _bool_plan, _clique_edges, _graph, _kcore
from test_gpu_louvain import _move
from test_gpu_lpa import _lpa
from test_gpu_match import _match
from test_gpu_msf import _msf
from test_gpu_scc import _scc
from test_gpu_truss import _truss
from test_louvain_cpu import move_loop
from test_lpa_cpu import greedy_colors, propagate
from test_match_cpu import greedy, pairs_of, pointer_rounds
from test_scc_cpu import scc_model

pytestmark = pytest.mark.gpu

N, PATH, K = 320, 300, 8                                    # the vertices 308 .. 319 are isolated
SWEEPS = 100
CALLS = ["kcore", "color", "color_prio", "truss", "msf", "match", "lpa", "louvain_move", "scc"]
ORDERS = [CALLS, ["scc", "msf", "lpa", "truss", "match", "color_prio", "louvain_move", "kcore", "color"]]
KNOBS = ("kcore_batch", "color_batch", "truss_batch", "msf_batch", "match_batch", "lpa_batch", "louvain_batch", "scc_batch")
# the index of the launch count in the stats
LAUNCHES = {"kcore": 3, "color": 2, "color_prio": 2, "truss": 3, "msf": 3, "match": 3, "lpa": 3, "louvain_move": 3, "scc": 4}
SCHEDULE = {"scc": 3}                                       # ... and of what else follows the hardware's schedule: gl_scc's rounds


@functools.lru_cache(maxsize=None)
def _inputs():
    v = np.arange(PATH)
    a, b = _clique_edges(K, PATH)
    sym = _graph(N, np.concatenate([v[:-1], [PATH - 1], a]), np.concatenate([v[1:], [PATH], b]))
    return sym, _random_prio(N, 3), np.arange(sym.nnz, dtype=np.float32), greedy_colors(sym)


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
    return {"match": (mate, (len(pairs_of(mate)), rounds, scans)), "lpa": (lpa[0], tuple(lpa[1:])),
            "louvain_move": (moved[0], tuple(moved[1:])), "scc": (scc[0], tuple(scc[1:4]))}


def _call(plan, call):
    """-> (the arrays to compare, the stats)"""
    sym, prio, weights, colors = _inputs()
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


def _without_launches(call, stats):
    return tuple(s for i, s in enumerate(stats) if i != LAUNCHES[call] and i != SCHEDULE.get(call))


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
    for call, (labels, stats) in models.items():
        assert np.array_equal(want[call][0][0], labels) and _without_launches(call, want[call][1]) == stats, call
    plan = _bool_plan(_inputs()[0])
    for order in ORDERS:
        for call in order:
            where = "%s in the order %s, batch %s" % (call, order, batch)
            arrays, stats = _call(plan, call)
            assert len(arrays) == len(want[call][0]) and all(np.array_equal(g, w) for g, w in zip(arrays, want[call][0])), where
            assert _without_launches(call, stats) == _without_launches(call, want[call][1]), where
            if call == "kcore":
                assert stats[3] >= 1 + 3 * stats[2], where
            if call in ("color", "color_prio"):
                assert (stats[2] - 2) % (2 * (batch or 64)) == 0 and stats[2] >= 2 + 2 * stats[1], where
                if batch == 1:
                    assert stats[2] == 2 + 2 * stats[1], where
