"""The round-based graph kernels share their host loop and the page-locked staging words their control records are read back
into (csrc/gl_rounds.h: rounds_run, csrc/gl_common.h: staging_words), and each keeps scratch in the plan: the outcome of a call
must not depend on which of them ran before it, on the same plan or through the same staging words.  On ONE plan gl_kcore,
gl_color (natural order and one priority array), gl_truss and gl_msf run in two different orders, with the four *_batch knobs at
1 -- many read-backs -- and at their defaults: every result array and every statistic but the launch count equals that of the
same call on a FRESH plan.  (The peeling order of gl_kcore is not unique: it is validated, not compared.)
The graph: a path of 300 vertices -- many rounds -- joined to a K_8 -- levels above 0, and triangles."""
import functools

import numpy as np
import pytest

from graphlily_amd import app

from helpers import set_knob
from test_gpu_coloring import _color, _random_prio
from test_gpu_kcore import _bool_plan, _clique_edges, _graph, _kcore
from test_gpu_msf import _msf
from test_gpu_truss import _truss

pytestmark = pytest.mark.gpu

N, PATH, K = 320, 300, 8                                    # the vertices 308 .. 319 are isolated
CALLS = ["kcore", "color", "color_prio", "truss", "msf"]
ORDERS = [CALLS, ["msf", "truss", "color_prio", "kcore", "color"]]
KNOBS = ("kcore_batch", "color_batch", "truss_batch", "msf_batch")
LAUNCHES = {"kcore": 3, "color": 2, "color_prio": 2, "truss": 3, "msf": 3}      # the index of the launch count in the stats


@functools.lru_cache(maxsize=None)
def _inputs():
    v = np.arange(PATH)
    a, b = _clique_edges(K, PATH)
    sym = _graph(N, np.concatenate([v[:-1], [PATH - 1], a]), np.concatenate([v[1:], [PATH], b]))
    return sym, _random_prio(N, 3), np.arange(sym.nnz, dtype=np.float32)


def _call(plan, call):
    """-> (the arrays to compare, the stats)"""
    sym, prio, weights = _inputs()
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
    forest, labels, stats = _msf(plan, weights, N)
    return (forest, labels), stats


def _without_launches(call, stats):
    return tuple(s for i, s in enumerate(stats) if i != LAUNCHES[call])


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
