"""The kernels that walk the plan's plain row copy share ONE skeleton (csrc/gl_rows.h: rows_walk_thread / rows_walk_takeover /
rows_walk_wave, launched through rows_walk_shape): a thread per row, four entries per step for `cut` entries, then the wavefront
takes the row over, 256 entries per step.  This file runs the skeleton's boundaries through every caller, so that a mistake in the
header fails under the header's name:
  all three templates   gl_cc_labels, gl_kcore, gl_color, gl_msf, gl_bfs_parents, gl_scc (over two plans) and gl_match, whose
                        collect kernel keeps a copy of the thread steps of its own
  takeover and wave     gl_lpa and gl_louvain_move, which count a row of at most 8 entries in registers instead of thread steps
  a copy of its own     gl_bc_accumulate, whose sweep walks the same way
The graph: a disjoint union of stars whose hub rows end on every side of a four-entry step, of the default cuts (8 and 32), of
the wavefront (64) and of the 256-entry takeover step.  In every star the hub has the LOWEST number and the leaf a check cares
about the HIGHEST, so that it is the last entry of the hub's row, in the row's last, partial group.  Each caller's cut runs over
0 (every row is taken over), 4 (exactly one thread step), 8 and its default; the expectations are closed forms, the validators of
app.py and the callers' host models.  gl_match and gl_scc deal a short list one row per wavefront and then have no thread steps,
gl_lpa and gl_louvain_move deal a colour class: their tests set the knobs and choose the inputs so that BOTH deals run, and say
in their docstrings why.  That the last entry of a hub row decides every one of their answers is proven without a GPU: the
*_stars() inputs below are run through the host models again with that entry (and its mirror) removed, in
tests/test_match_cpu.py, test_scc_cpu.py, test_lpa_cpu.py and test_louvain_cpu.py."""
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
from test_gpu_kcore import _bool_plan, _graph, _kcore, _sorted_rows
from test_gpu_louvain import _move
from test_gpu_lpa import _lpa
from test_gpu_match import _match
from test_gpu_msf import _msf
from test_gpu_scc import _scc
from test_kcore_cpu import _csr
from test_louvain_cpu import move_loop
from test_lpa_cpu import propagate
from test_match_cpu import FREE, greedy, mate_of_pairs, pairs_of, pointer_rounds
from test_msf_cpu import graph_of, ones_of
from test_scc_cpu import scc_model

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


# ------------------------------------------------------------------ gl_match, gl_scc, gl_lpa, gl_louvain_move: the star inputs
# Built and answered by the host models on the CPU, once, shared, never written.  `drop` is for the CPU suites' proof that one
# entry of a hub row decides the answer: "last" ("first") removes every hub's last (first) entry and its mirror from the graph.
def _star_edges(drop=None):
    """-> (hub, leaf, kept) of every star edge, ascending by leaf: inside a star in the order of the hub's row"""
    hub_of, last = _stars()[2], _stars()[4]
    leaf = np.flatnonzero((hub_of >= 0) & (hub_of != np.arange(N)))
    hub = hub_of[leaf]
    assert drop in (None, "last", "first")
    kept = ~np.isin(leaf, last) if drop == "last" else leaf != hub + 1 if drop == "first" else np.ones(leaf.shape[0], bool)
    assert np.count_nonzero(~kept) == (0 if drop is None else 17)
    return hub, leaf, kept


def star_hubs(at_least):
    """the hubs with at least that many leaves"""
    return _stars()[3][np.asarray(DEGREES) >= at_least]


def _frozen(*arrays):
    for arr in arrays:
        if arr is not None:
            arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def match_stars(ascending, drop=None):
    """distinct whole weights, ascending (descending) inside each star: the hub's heaviest edge is its LAST (FIRST) entry
    -> (the weighted symmetric matrix, pointer_rounds()'s mates == greedy()'s, rounds, scans)"""
    hub, leaf, kept = _star_edges(drop)
    w = np.arange(1, hub.shape[0] + 1) if ascending else np.arange(hub.shape[0], 0, -1)
    sym = graph_of(N, hub[kept], leaf[kept], w[kept])
    mate, rounds, scans = pointer_rounds(sym)
    assert np.array_equal(mate, greedy(sym))
    _frozen(mate, sym.adj_data, sym.adj_indices, sym.adj_indptr)
    return sym, mate, rounds, scans


@functools.lru_cache(maxsize=None)
def scc_stars(kind, loops=False, prio=False, drop=None):
    """kind "in":  every leaf -> its hub, and hub -> its highest leaf only: the long rows are plan_in's (the predecessors)
            "out": the same with every edge turned round: the long rows are plan_out's (the successors)
            "sym": both directions of every star edge, declared symmetric (plan_out is None)
    loops: an entry (v, v) in every leaf's rows -- gl_scc ignores it when it walks, but the row is not empty, so the leaf is live
    when the first pass begins and is on its list (the model gets the edges without the loops: it is stated for simple graphs).
    prio: the highest leaf of every star has the top priority.  `drop` removes the long row's last entry: the edge between the
    highest leaf and the hub in that row's direction (both directions for "sym").
    -> (csr_in, csr_out or None, priorities or None, scc_model()'s (labels, components, passes, trimmed, rounds))"""
    hub, leaf, kept = _star_edges(drop)
    hubs, last = star_hubs(1), _stars()[4]
    if kind == "sym":
        src, dst = np.concatenate([leaf[kept], hub[kept]]), np.concatenate([hub[kept], leaf[kept]])
    else:
        src, dst = np.concatenate([leaf[kept], hubs]), np.concatenate([hub[kept], last])
        if kind == "out":
            src, dst = dst, src
    own = leaf if loops else leaf[:0]
    cin = _sorted_rows(_csr(N, np.concatenate([dst, own]), np.concatenate([src, own])))      # an entry A[v, u] is the edge u -> v
    cout = None if kind == "sym" else _sorted_rows(_csr(N, np.concatenate([src, own]), np.concatenate([dst, own])))
    p = None
    if prio:
        p = np.zeros(N, np.uint32)
        p[last] = 1
    want = scc_model(N, src, dst, p)
    _frozen(want[0], p, cin.adj_indices, cin.adj_indptr)
    return cin, cout, p, want


def _star_colors(packed):
    """hubs 0, leaves 1; the 24 vertices without a neighbour (the hub without leaves, the 23 behind the stars) go with the hubs
    (packed) or with the leaves"""
    hub_of = _stars()[2]
    colors = ((hub_of >= 0) & (hub_of != np.arange(N))).astype(np.uint32)
    colors[hub_of < 0] = 0 if packed else 1
    assert np.count_nonzero(colors == 0) == (17 + 24 if packed else 17)
    return colors


@functools.lru_cache(maxsize=None)
def lpa_stars(packed=False, drop=None):
    """initial labels: own numbers, except that each star's FIRST leaf starts with its HIGHEST leaf's number -- the largest label of
    the hub's row, so no tie rule picks it, and it is counted twice only if the row's last entry is counted
    -> (the symmetric pattern, colours, initial labels, propagate()'s (labels, sweeps, changes, evaluations, converged))"""
    hub, leaf, kept = _star_edges(drop)
    sym = _graph(N, hub[kept], leaf[kept])
    colors = _star_colors(packed)
    init = np.arange(N, dtype=np.uint32)
    init[star_hubs(1) + 1] = _stars()[4]
    want = propagate(sym, colors, init, 10)
    _frozen(want[0], colors, init)
    return sym, colors, init, want


def _louvain_weights(sym, heavy):
    """1 for every entry but the two between a hub and its highest leaf"""
    rows = np.repeat(np.arange(N), np.diff(sym.adj_indptr.astype(np.int64)))
    last = _stars()[4]
    return np.where(np.isin(rows, last) | np.isin(sym.adj_indices, last), heavy, 1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def louvain_stars(packed=False, drop=None):
    """unit weights, except hub -- highest leaf: the smallest whole weight with which move_loop() moves every hub with two leaves
    or more into its highest leaf's community in sweep 1 (found here, on the whole graph; among equal scores the hub would take
    its FIRST leaf, the smallest label)
    -> (the symmetric pattern, entry weights, colours, that weight, move_loop() after one sweep, move_loop() at its end)"""
    hub, leaf, kept = _star_edges(drop)
    sym = _graph(N, hub[kept], leaf[kept])
    colors = _star_colors(packed)
    hubs, last = star_hubs(2), _stars()[4][np.asarray(DEGREES)[np.asarray(DEGREES) > 0] >= 2]
    if drop is not None:
        heavy = louvain_stars(packed)[3]
    else:
        for heavy in range(2, 10):
            label = move_loop(sym, _louvain_weights(sym, heavy), None, colors, 1, 0)[0]
            if np.array_equal(label[hubs], label[last]):
                break
        else:
            raise AssertionError("no weight up to 9 moves every hub to its highest leaf in sweep 1")
    weights = _louvain_weights(sym, heavy)
    first, full = move_loop(sym, weights, None, colors, 1, 0), move_loop(sym, weights, None, colors, 20, 0)
    _frozen(weights, colors, first[0], full[0])
    return sym, weights, colors, heavy, first, full


# ------------------------------------------------------------------ ... and their tests
MATCH_CUTS = [0, 4, 8, None, 64]
SCC_DEALS = [(True, 0), (True, 4), (True, None), (True, 32), (False, None)]
CLASS_CUTS = [0, 4, None]


@pytest.mark.parametrize("ascending", [True, False], ids=["last_entry_heaviest", "first_entry_heaviest"])
@pytest.mark.parametrize("spread", [0, None], ids=["64_rows_per_wavefront", "row_per_wavefront"])
@pytest.mark.parametrize("cut", MATCH_CUTS)
def test_match(gpu, monkeypatch, cut, spread, ascending):
    """The deal.  A point or collect launch has max(rows_walk_shape's cdiv(2560, 256) = 10, min(8 x CUs, cdiv(2560, 4) = 640))
    = 640 workgroups on any device with 80 compute units or more: 2560 wavefronts.  Round 1 lists the 2536 vertices with a row,
    round 2 the 2502 leaves that must point again, and a collect gets the 34 fresh vertices: each list has at most one row per
    wavefront, so match_deal spreads it down to ONE row per wavefront and drops the thread steps -- unless that is more than
    match_spread allows.  match_spread=0 allows nothing: 64 rows per wavefront (40, 40 and 1 words), a thread per row for `cut`
    entries; the default (16) gives a row per wavefront, whatever the cut.
    The answer.  Every leaf points at its hub, the hub at its heaviest edge -- its LAST entry (its FIRST in the second variant,
    which catches an off-by-one at the row's front): 17 pairs in round 1.  Round 2 scans the other 2519 - 17 leaves, which find
    nobody.  The scans are what catches the collect kernel's own copy of the thread steps: a leaf that the hub's walk misses is
    never listed again, and the matching itself does not show it."""
    set_knob(monkeypatch, "match_cut", cut)
    set_knob(monkeypatch, "match_spread", spread)
    sym, want, rounds, scans = match_stars(ascending)
    hubs, last = star_hubs(1), _stars()[4]
    assert np.array_equal(want, mate_of_pairs(N, hubs, last if ascending else hubs + 1)) and np.count_nonzero(want == FREE) == N - 34
    assert (len(pairs_of(want)), rounds, scans) == (17, 2, 2536 + 2519 - 17)
    plan = _bool_plan(ones_of(sym))
    for _ in range(2):
        mate, stats = _match(plan, sym.adj_data, N)
        assert np.array_equal(mate, want)
        assert stats[:3] == (17, rounds, scans)


@pytest.mark.parametrize("prio", [False, True], ids=["natural", "highest_leaf_first"])
@pytest.mark.parametrize("kind", ["in", "out"])
@pytest.mark.parametrize("loops,cut", SCC_DEALS)
def test_scc_directed(gpu, monkeypatch, loops, cut, kind, prio):
    """The deal.  A round launch has rows_walk_shape's cdiv(2560, 256) = 10 workgroups (scc_grid cannot make it fewer): 40
    wavefronts, and scc_deal gives each ceil(listed / 40) vertices, 64 at most; with ONE it drops the thread steps.  Pass 1 lists
    the vertices whose two rows both have an entry.  Without the loops these are the 17 hubs and their 17 highest leaves: 34, a
    row per wavefront, whatever the cut.  With a loop in every leaf's rows they are 2519 + 17 = 2536: 64 per wavefront (40
    words), a thread per row for scc_cut entries.
    The answer.  kind "in": the hub's row of plan_in holds all its leaves; all but the highest have no predecessor and are
    trimmed (when the list is made, or in the first trim round), so the hub survives only if its walk over its predecessors
    finds the one live entry, the LAST.  Under the priorities the highest leaf is the root, and the forward minimum reaches the
    hub through the same entry.  kind "out": the long rows are plan_out's; the successor trim has to find the last entry, and
    under the priorities so has the backward walk of the hub, which is then no root.
    Hub and highest leaf are one component, everybody else is alone: N - 17 components in one pass.  (`trimmed` is more than the
    sum of d - 1 over the stars, 2519 - 17: the hub without leaves and the 23 vertices behind the stars are components of their
    own too, and scc_model, the authority here, counts them as trimmed as the kernel does: 24 more.)"""
    set_knob(monkeypatch, "scc_cut", cut)
    cin, cout, p, (lab, comps, passes, trimmed, rounds) = scc_stars(kind, loops, prio)
    hubs, last = star_hubs(1), _stars()[4]
    want = np.arange(N)
    want[last] = hubs
    assert np.array_equal(lab, want) and (comps, passes, trimmed) == (N - 17, 1, 2519 - 17 + 24)
    live = (np.diff(cin.adj_indptr.astype(np.int64)) > 0) & (np.diff(cout.adj_indptr.astype(np.int64)) > 0)
    assert np.count_nonzero(live) == (2536 if loops else 34)
    assert np.array_equal(np.diff((cin if kind == "in" else cout).adj_indptr.astype(np.int64))[_stars()[3]], DEGREES)
    pin, pout = _bool_plan(cin), _bool_plan(cout)
    for _ in range(2):
        got, stats = _scc(pin, pout, N, p)
        assert np.array_equal(got, lab)
        assert stats[:3] == (comps, passes, trimmed) and passes <= stats[3] <= rounds


@pytest.mark.parametrize("cut", [0, 4, None, 32])
def test_scc_symmetric_with_priorities(gpu, monkeypatch, cut):
    """Symmetric stars, one plan.  Pass 1 lists the 2536 vertices with a row: ceil(2536 / 40) = 64 per wavefront (there is no
    input on these stars that lists 40 or fewer: the row-per-wavefront deal is test_scc_directed's).  The highest leaf has the top
    priority, so the forward minimum must reach the hub through its LAST entry -- otherwise that leaf is collected alone and keeps
    its own number.  Labels are the hubs."""
    set_knob(monkeypatch, "scc_cut", cut)
    cin, cout, p, (lab, comps, passes, trimmed, rounds) = scc_stars("sym", False, True)
    hub_of = _stars()[2]
    assert cout is None and np.array_equal(lab, np.where(hub_of >= 0, hub_of, np.arange(N)))
    assert (comps, passes, trimmed) == (len(DEGREES) + N - 2537, 1, 1 + N - 2537)
    pin = _bool_plan(cin)
    for _ in range(2):
        got, stats = _scc(pin, None, N, p)
        assert np.array_equal(got, lab)
        assert stats[:3] == (comps, passes, trimmed) and passes <= stats[3] <= rounds


def _star_members():
    """-> (the vertices of the stars with a leaf, the highest leaf of each one's star)"""
    hub_of = _stars()[2]
    highest = np.full(N, -1, np.int64)
    highest[star_hubs(1)] = _stars()[4]
    members = np.flatnonzero(hub_of >= 0)
    return members, highest[hub_of[members]]


@pytest.mark.parametrize("table", [None, 8])
@pytest.mark.parametrize("packed", [False, True], ids=["row_per_wavefront", "two_rows_per_wavefront"])
@pytest.mark.parametrize("cut", CLASS_CUTS)
def test_lpa(gpu, monkeypatch, cut, packed, table):
    """The deal.  A class launch has rows_walk_shape's cdiv(2560, 256) = 10 workgroups: 40 wavefronts, each with ceil(class / 40)
    vertices, 64 at most.  The hubs are colour 0.  Alone they are 17: a row per wavefront.  With the 24 vertices without a neighbour
    they are 41: two per wavefront, 21 words.  (64 hubs per wavefront would take a class above 2520 on 2560 vertices; a hub's
    leaves cannot be in its class.)  Unlike gl_scc and gl_match, gl_lpa keeps its thread path under either deal: a row of at most
    lpa_cut <= 8 entries is counted in registers, every longer one by the wavefront; the leaves, 63 or 64 to a wavefront, are
    thread rows, or 64 one-entry takeovers at cut 0.  lpa_table=8: the rows of 9 entries and more, and with them those of 255,
    256, 257 and 545, are counted partition by partition.
    The answer.  Sweep 1, class 0: the hub's row holds its highest leaf's number twice -- first entry and LAST -- and every other
    label once, so the hub takes it iff the last entry is counted; class 1: every leaf follows its hub.  Sweep 2 changes
    nothing."""
    set_knob(monkeypatch, "lpa_cut", cut)
    set_knob(monkeypatch, "lpa_table", table)
    sym, colors, init, (lab, sweeps, changes, evals, converged) = lpa_stars(packed)
    members, highest = _star_members()
    want = np.arange(N)
    want[members] = highest
    # (everybody in a star changes once, but its highest leaf and, where that is another vertex, the first leaf that began with its label)
    assert np.array_equal(lab, want) and (sweeps, converged) == (2, 1) and changes == members.shape[0] - 17 - 16
    plan = _bool_plan(sym)
    for _ in range(2):
        got, stats = _lpa(plan, N, colors, init, 10)
        assert np.array_equal(got, lab)
        assert (stats[0], stats[1], stats[2], stats[4]) == (sweeps, changes, evals, converged)


@pytest.mark.parametrize("table", [None, 8])
@pytest.mark.parametrize("packed", [False, True], ids=["row_per_wavefront", "two_rows_per_wavefront"])
@pytest.mark.parametrize("cut", CLASS_CUTS)
def test_louvain_move(gpu, monkeypatch, cut, packed, table):
    """The deal is gl_lpa's (test_lpa): 17 hubs in class 0 are a row per wavefront, 41 vertices two, and the thread path -- rows of
    at most louvain_cut <= 8 entries -- runs under both.  louvain_table=8 sums the longer rows partition by partition.
    The answer.  Sweep 1, class 0: towards every leaf but the highest the hub's score is the same, towards the highest it is
    `heavy` times that, so the hub joins its highest leaf iff its LAST entry is summed (and its first leaf otherwise).  The
    vertex weights are sums over the rows too: an entry lost there changes two_m and every score."""
    set_knob(monkeypatch, "louvain_cut", cut)
    set_knob(monkeypatch, "louvain_table", table)
    sym, weights, colors, heavy, first, full = louvain_stars(packed)
    hubs, last = star_hubs(2), _stars()[4][1:]
    assert heavy == 2 and np.array_equal(first[0][hubs], last) and np.array_equal(full[0][hubs], last)
    plan = _bool_plan(sym)
    for _ in range(2):
        got, stats = _move(plan, N, weights, None, colors, 1, 0)
        assert np.array_equal(got[hubs], got[last]) and np.array_equal(got, first[0])
        assert stats[:3] + stats[4:] == tuple(first[1:])
        got, stats = _move(plan, N, weights, None, colors, 20, 0)
        assert np.array_equal(got, full[0])
        assert stats[:3] + stats[4:] == tuple(full[1:])
