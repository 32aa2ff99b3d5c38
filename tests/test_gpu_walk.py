"""The kernels that walk the plan's plain row copy share ONE skeleton (csrc/gl_rows.h: rows_walk_thread / rows_walk_takeover /
rows_walk_wave, launched through rows_walk_shape): a thread per row, four entries per step for `cut` entries, then the wavefront
takes the row over, 256 entries per step.  This file runs the skeleton's boundaries through every caller -- gl_cc_labels, gl_kcore,
gl_color, gl_msf, gl_bfs_parents -- so that a mistake in the header fails under the header's name, and through gl_bc_accumulate,
whose sweep walks the same way in a copy of its own.
The graph: a disjoint union of stars whose hub rows end on every side of a four-entry step, of the default cuts (8 and 32), of
the wavefront (64) and of the 256-entry takeover step.  In every star the hub has the LOWEST number and the leaf a check cares
about the HIGHEST, so that it is the last entry of the hub's row, in the row's last, partial group.  Each caller's cut runs over
0 (every row is taken over), 4 (exactly one thread step), 8 and its default; the expectations are closed forms and the
validators of app.py."""
import functools

import numpy as np
import pytest

from graphlily_amd import app

from helpers import set_knob
from test_bc_cpu import assert_close, bound_of
from test_gpu_bc import _bc, _host
from test_gpu_bfs_parents import _run_plan
from test_gpu_cc import _labels_of
from test_gpu_coloring import _color, _random_prio
from test_gpu_kcore import _bool_plan, _graph, _kcore
from test_gpu_msf import _msf
from test_msf_cpu import graph_of, ones_of

pytestmark = pytest.mark.gpu

DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257, 8 + 256, 8 + 257, 32 + 512, 32 + 513]
N = 2560                                                    # 2537 vertices of stars (2519 leaves and 18 hubs), 23 isolated ones behind them
CUTS = [0, 4, 8, None]
NONE = 0xffffffff


@functools.lru_cache(maxsize=None)
def _stars():
    """-> (the symmetric pattern, the same with distinct weights, hub of every vertex or -1, hubs, highest leaves); shared, never
    written.  Star i is the hub hubs[i] and the leaves hubs[i] + 1 .. hubs[i] + DEGREES[i]."""
    hubs = np.cumsum([0] + [d + 1 for d in DEGREES[:-1]])
    assert hubs[-1] + DEGREES[-1] + 1 == 2537 <= N
    a = np.concatenate([np.full(d, h) for h, d in zip(hubs, DEGREES)])
    b = np.concatenate([h + 1 + np.arange(d) for h, d in zip(hubs, DEGREES)])
    hub_of = np.full(N, -1, np.int64)
    hub_of[a], hub_of[b] = a, a
    sym = _graph(N, a, b)
    # distinct weights (whole numbers, exact in f32), descending inside a star: the hub's lightest edge is its LAST entry
    weighted = graph_of(N, a, b, np.arange(a.shape[0], 0, -1))
    assert sym.nnz == weighted.nnz == 2 * a.shape[0] and np.array_equal(sym.adj_indices, weighted.adj_indices)
    assert np.array_equal(np.diff(sym.adj_indptr.astype(np.int64))[hubs], DEGREES)
    for arr in (hub_of, hubs):
        arr.setflags(write=False)
    last = hubs + np.asarray(DEGREES)
    return sym, weighted, hub_of, hubs, last[np.asarray(DEGREES) > 0]


def _levels(sources):
    sym = _stars()[0]
    level = app._bfs_levels_of(app._pattern_as_scipy(sym, N), sources, N)
    level.setflags(write=False)
    return level


@pytest.mark.parametrize("cut", CUTS)
def test_cc_labels(gpu, monkeypatch, cut):
    set_knob(monkeypatch, "cc_cut", cut)
    sym, _, hub_of, _, _ = _stars()
    labels, count = _labels_of(_bool_plan(sym), N)
    want = np.where(hub_of >= 0, hub_of, np.arange(N))
    assert np.array_equal(labels, want)
    assert count == len(DEGREES) + (N - 2537) == app.validate_components(sym, labels)


@pytest.mark.parametrize("cut", CUTS)
def test_kcore(gpu, monkeypatch, cut):
    set_knob(monkeypatch, "kcore_cut", cut)
    sym = _stars()[0]
    core, order, stats = _kcore(_bool_plan(sym), N)
    assert np.array_equal(core, (np.diff(sym.adj_indptr.astype(np.int64)) > 0).astype(np.uint32))
    assert app.validate_cores(sym, core, order) == stats[0] == 1


@pytest.mark.parametrize("prio", [False, True])
@pytest.mark.parametrize("cut", CUTS + [64])
def test_color(gpu, monkeypatch, cut, prio):
    set_knob(monkeypatch, "color_cut", cut)
    sym, _, hub_of, _, _ = _stars()
    priorities = _random_prio(N, 5) if prio else None
    colours, stats = _color(_bool_plan(sym), N, priorities)
    assert app.validate_coloring(sym, colours, priorities) == stats[0] == 2
    if not prio:                                            # natural order: the hub goes before its leaves
        assert np.array_equal(colours, ((hub_of >= 0) & (hub_of != np.arange(N))).astype(np.uint32))


@pytest.mark.parametrize("cut", CUTS)
def test_msf(gpu, monkeypatch, cut):
    set_knob(monkeypatch, "msf_cut", cut)
    _, weighted, hub_of, _, _ = _stars()
    forest, labels, stats = _msf(_bool_plan(ones_of(weighted)), weighted.adj_data, N)
    assert np.array_equal(forest, np.ones(weighted.nnz, np.uint32))            # a forest with distinct weights: every edge
    assert stats[0] == weighted.nnz // 2 == app.validate_spanning_forest(weighted, forest)
    assert stats[1] == len(DEGREES) + (N - 2537) and np.array_equal(labels, np.where(hub_of >= 0, hub_of, np.arange(N)))


@pytest.mark.parametrize("early", [None, 0])
@pytest.mark.parametrize("cut", CUTS)
def test_bfs_parents(gpu, monkeypatch, cut, early):
    """early = None: the rows ascend, so the first match ends a row; 0: the full scan"""
    set_knob(monkeypatch, "parents_cut", cut)
    set_knob(monkeypatch, "parents_early", early)
    sym, _, hub_of, hubs, last = _stars()
    plan = _bool_plan(sym)
    # from the highest leaf of the largest star: its hub one step away, the other leaves two
    source, hub = int(last[-1]), int(hubs[-1])
    level = _levels([source])
    want_level = np.zeros(N, np.float32)
    want_level[hub_of == hub] = 3.0
    want_level[hub], want_level[source] = 2.0, 1.0
    assert np.array_equal(level, want_level)
    parent, orphans = _run_plan(plan, level)
    want = np.where(hub_of == hub, hub, NONE).astype(np.uint32)
    want[hub] = want[source] = source
    assert orphans == 0 and np.array_equal(parent, want)
    assert app.validate_bfs_tree(sym, source, level, parent) == DEGREES[-1] + 1
    # from the highest leaf of EVERY star at once: every hub row has to find its last entry
    level = _levels(last)
    parent, orphans = _run_plan(plan, level)
    want = np.where(hub_of >= 0, hub_of, NONE).astype(np.uint32)
    want[hubs[np.asarray(DEGREES) > 0]] = last
    want[last] = last
    want[hubs[0]] = NONE                                    # the star without leaves is not reached
    assert orphans == 0 and np.array_equal(parent, want)


@pytest.mark.parametrize("cut", CUTS)
def test_bc_accumulate(gpu, monkeypatch, cut):
    set_knob(monkeypatch, "bc_cut", cut)
    sym, _, _, hubs, last = _stars()
    plan = _bool_plan(sym)
    source, hub = int(last[-1]), int(hubs[-1])
    bc, sigma, stats = _bc(plan, plan, _levels([source]), scale=app._bc_scale(N, 1, False, False))
    assert stats == (3, DEGREES[-1] + 1, 0, 0) and np.count_nonzero(bc) == 1 and bc[hub] > 0
    app.validate_betweenness(sym, bc, sources=[source])     # (its own bound: the one test_gpu_bc.py uses, from depth and longest row)
    # the highest leaf of every star at level 1: every hub's sums run over its whole row, forward (one path) and backward
    level = _levels(last)
    host_sigma, host_bc, _ = _host(sym, None, level)
    bc, sigma, stats = _bc(plan, plan, level)
    assert stats == (3, 2537 - 1, 0, 0) and np.array_equal(sigma, host_sigma)
    assert_close(bc, host_bc, bound_of(3, max(DEGREES), 1), "every star")
    assert np.array_equal(bc[hubs], np.maximum(np.asarray(DEGREES, np.float64) - 1.0, 0.0))
