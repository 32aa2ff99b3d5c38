"""CPU suite of label propagation communities (gl_lpa, SpMVPlan.lpa, SpMVModule.lpa, app.LabelPropagation,
app.validate_communities, io.lpa_initial_labels): the export and its bindings exist; the host truth kept here -- propagate(), a
dictionary loop over the vertices in (colour, vertex) order, or over all of them from the previous sweep's labels -- gives the closed
forms of cliques, stars, K_{5,7} and paths, keeps both invariants (every change raises the number of edges whose ends share a label;
a converged run is a fixed point), counts as evaluations exactly the evaluations that saw a changed neighbour, and agrees with
app._lpa_color_loop on every graph tests/test_gpu_lpa.py uses; the validator accepts the truth and refuses one violation per rule;
the driver refuses what it cannot do, and the C++ driver compiles against include/.
tests/test_gpu_lpa.py compares the kernels with propagate() (kept here) bit for bit."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver, named_matrix
from test_msf_cpu import clique_edges, entry_rows, raw_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LPA_DRIVER = os.path.join(ROOT, "build", "lpa_driver")
HEADER = "graphlily_hip_lpa.h"
DECL = ("int gl_lpa(gl_spmv_plan plan, const uint32_t *d_color /* may be NULL: synchronous */, const uint32_t *d_init /* may be NULL: own "
        "number */, uint32_t *d_label, uint32_t max_sweeps, uint64_t *h_stats /* may be NULL, 5 words: sweeps, changes, evaluations, "
        "launches, converged */);")
TOP = 0xfffffffe                      # the largest label there is: 0xffffffff is reserved


# ------------------------------------------------------------------ the host truth
def _hoods(sym):
    indptr = sym.adj_indptr.astype(np.int64).tolist()
    cols = sym.adj_indices.astype(np.int64).tolist()
    return [[u for u in cols[indptr[v]:indptr[v + 1]] if u != v] for v in range(sym.num_rows)]


def _evaluate(label, hood, own):
    """the rule -> the label v carries after its evaluation"""
    cnt = {}
    for u in hood:
        cnt[label[u]] = cnt.get(label[u], 0) + 1
    best = max(cnt.values())
    return min(l for l, c in cnt.items() if c == best) if best > cnt.get(own, 0) else own


def propagate(sym, colors, init, max_sweeps, synchronous=False, on_change=None, use_active=True):
    """-> (uint32[n] labels, sweeps, changes, evaluations, converged).  colors: a proper colouring (ignored when synchronous);
    init: n labels or None for own numbers.  on_change(v, old, new, label) is called before every change of the in-place
    schedule; use_active=False evaluates every vertex with a neighbour in every sweep."""
    n = sym.num_rows
    hood = _hoods(sym)
    label = list(range(n)) if init is None else [int(x) for x in init]
    linked = [v for v in range(n) if hood[v]]
    if not synchronous:
        col = [int(c) for c in colors]
        linked.sort(key=lambda v: (col[v], v))
    active = [bool(h) for h in hood]
    sweeps = changes = evaluations = converged = 0
    while sweeps < max_sweeps and not converged:
        sweeps += 1
        changed = 0
        source = list(label) if synchronous else label
        woken = [False] * n if synchronous else active
        for v in linked:
            if use_active and not active[v]:
                continue
            active[v] = False
            evaluations += 1
            new = _evaluate(source, hood[v], source[v])
            if new != source[v]:
                if on_change:
                    on_change(v, source[v], new, label)
                label[v] = new
                changed += 1
                for u in hood[v]:
                    woken[u] = True
        if synchronous:
            active = woken
        changes += changed
        converged = int(changed == 0)
    return np.asarray(label, dtype=np.uint32), sweeps, changes, evaluations, converged


def greedy_colors(sym, prio=None):
    """first-fit greedy in gl_color's order: larger priority first, ties to the smaller vertex number -> uint32[n]"""
    n = sym.num_rows
    hood = _hoods(sym)
    order = range(n) if prio is None else sorted(range(n), key=lambda v: (-int(prio[v]), v))
    color = [-1] * n
    for v in order:
        used = {color[u] for u in hood[v]}
        c = 0
        while c in used:
            c += 1
        color[v] = c
    return np.asarray(color, dtype=np.uint32)


def same_label_edges(sym, label):
    rows, cols = entry_rows(sym), sym.adj_indices.astype(np.int64)
    lab = np.asarray(label)
    return int(np.count_nonzero((lab[rows] == lab[cols]) & (rows < cols)))


def is_fixed_point(sym, label):
    hood = _hoods(sym)
    lab = [int(x) for x in label]
    return all(_evaluate(lab, h, lab[v]) == lab[v] for v, h in enumerate(hood) if h)


# ------------------------------------------------------------------ the graphs of tests/test_gpu_lpa.py
def simple_graph(n, a, b):
    return io.symmetrize_simple(raw_csr(n, a, b, np.ones(len(a))))[0]


def path_graph(shuffled):
    """a path through the first 600 of 640 vertices: 0 - 1 - ... - 599, or the same vertices in a fixed random order"""
    walk = np.random.default_rng(5).permutation(600) if shuffled else np.arange(600)
    return simple_graph(640, walk[:-1], walk[1:])


def cliques_graph(k):
    """three disjoint K_k, the first on 5 .. k + 4, two unused vertices between them"""
    a, b = zip(*[clique_edges(k, 5 + i * (k + 2)) for i in range(3)])
    return simple_graph(-(-(3 * (k + 2) + 5) // 128) * 128, np.concatenate(a), np.concatenate(b))


def star_graph():
    """hub 7, leaves 8 .. 607"""
    return simple_graph(640, np.full(600, 7), np.arange(8, 608))


def hubs_graph():
    """hubs 0 and 1, not adjacent, over the leaves 2 .. 301"""
    leaves = np.arange(2, 302)
    return simple_graph(384, np.concatenate([np.zeros(300, np.int64), np.ones(300, np.int64)]), np.concatenate([leaves, leaves]))


def bipartite_graph():
    """K_{5,7} on 3 .. 7 and 20 .. 26"""
    a, b = np.meshgrid(np.arange(3, 8), np.arange(20, 27))
    return simple_graph(128, a.ravel(), b.ravel())


# one star per branch of the rule: (centre, its initial label, the leaves' initial labels, the centre's label after sweep 1)
BRANCHES = [
    (10, 3, [5, 5, 9, 9], 5),                         # a tie that excludes the current label takes the smallest; cur = 0
    (20, 9, [5, 5, 9, 9], 9),                         # a tie that includes the current label keeps it
    (30, 9, [5, 5, 5, 9, 9], 5),                      # a strict gain moves the vertex
    (40, 9, [5, 7, 9], 9),                            # all counts 1, the current label among them: it stays
    (50, 2, [TOP, TOP, 7], TOP),                      # labels up to 0xfffffffe
    (60, TOP, [TOP - 1, 1, TOP - 1], TOP - 1),
    (70, 0, [4] * 9 + [6] * 9 + [0] * 8, 4),          # a row the wavefront counts: 9 : 9 : 8, cur = 8
    (100, 6, [4] * 9 + [6] * 9 + [0] * 8, 6),         # the same row with the current label in the tie
]


def branches_graph():
    """-> (graph, colours, initial labels, {centre: label after one sweep}): the stars of BRANCHES, centres in class 0, leaves in
    class 1; the initial labels are not injective"""
    n = 256
    a, b, init, want = [], [], np.arange(n, dtype=np.uint32), {}
    colors = np.zeros(n, dtype=np.uint32)
    for centre, own, leaves, after in BRANCHES:
        init[centre] = own
        want[centre] = after
        for i, l in enumerate(leaves):
            a.append(centre)
            b.append(centre + 1 + i)
            init[centre + 1 + i] = l
            colors[centre + 1 + i] = 1
    return simple_graph(n, a, b), colors, init, want


def planted_graph():
    """20 blocks of 60 vertices, p_in 0.3, p_out 0.005, on 1280 vertices (the last 80 unused)"""
    rng = np.random.default_rng(20)
    iu = np.triu_indices(1200, 1)
    same = iu[0] // 60 == iu[1] // 60
    keep = rng.random(iu[0].shape[0]) < np.where(same, 0.3, 0.005)
    return simple_graph(1280, iu[0][keep], iu[1][keep])


def largest_first(sym, seed=0):
    deg = np.diff(sym.adj_indptr.astype(np.int64)).astype(np.uint32)
    return greedy_colors(sym, io.coloring_priorities(deg, "largest_first", seed))


@functools.lru_cache(maxsize=None)
def lpa_case(name):
    """-> (graph, colours or None, initial labels or None, max_sweeps, (labels, sweeps, changes, evaluations, converged)): computed
    once, shared, never written.  A name "sync_<graph>_<max_sweeps>" is the synchronous schedule."""
    init, max_sweeps, sync = None, 100, name.startswith("sync_")
    if sync:
        _, graph, cap = name.split("_")
        max_sweeps = int(cap)
        sym = {"bipartite": bipartite_graph, "path": lambda: path_graph(False), "clique": lambda: cliques_graph(17)}[graph]()
        colors = None
    elif name == "path_2":
        sym = path_graph(False)
        colors = (np.arange(640) % 2).astype(np.uint32)
    elif name == "path_natural":
        sym = path_graph(True)
        colors = greedy_colors(sym)
    elif name.startswith("cliques_"):
        sym = cliques_graph(int(name[8:]))
        colors = greedy_colors(sym)
    elif name == "star":
        sym = star_graph()
        colors = largest_first(sym)
    elif name == "hubs":
        sym = hubs_graph()
        colors = largest_first(sym)
    elif name == "bipartite":
        sym = bipartite_graph()
        colors = greedy_colors(sym)
    elif name in ("branches_1", "branches"):
        sym, colors, init, _ = branches_graph()
        max_sweeps = 1 if name == "branches_1" else 100
    elif name in ("planted", "planted_short", "planted_seeded"):
        sym = planted_graph()
        colors = largest_first(sym)
        if name == "planted_short":
            max_sweeps = lpa_case("planted")[4][1] - 1
        if name == "planted_seeded":
            init = io.lpa_initial_labels(1200, 3, 1280)
    elif name == "rmat":
        raw = named_matrix("rmat_20K")
        io.util_round_csr_matrix_dim(raw, 128, 128)
        sym = io.symmetrize_simple(raw)[0]
        colors = largest_first(sym)
    else:
        raise KeyError(name)
    want = propagate(sym, colors, init, max_sweeps, sync)
    want[0].setflags(write=False)
    for arr in (colors, init):
        if arr is not None:
            arr.setflags(write=False)
    return sym, colors, init, max_sweeps, want


COLOR_CASES = ["path_2", "path_natural", "cliques_3", "cliques_17", "cliques_65", "cliques_130", "star", "hubs", "bipartite", "branches_1",
               "branches", "planted", "planted_short", "planted_seeded", "rmat"]
SYNC_CASES = ["sync_bipartite_6", "sync_bipartite_7", "sync_path_6", "sync_path_7", "sync_clique_100"]


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_lpa"), "libgraphlily_hip.so does not export gl_lpa"
    assert len(L.gl_lpa.argtypes) == 6
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_lpa"]
    assert capi.EXT_HEADERS["graphlily_hip_lpa.h"] == ["gl_lpa"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_lpa" not in capi.EXPORTS and "gl_lpa" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.lpa) and callable(M.SpMVModule.lpa)
    assert callable(app.LabelPropagation.run) and callable(app.LabelPropagation.modularity) and callable(app.validate_communities)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void lpa(DeviceBuffer label, const uint32_t *color = nullptr, const uint32_t *init = nullptr, uint32_t max_sweeps = 100," in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    lpa_h = open(os.path.join(ROOT, "include", "graphlily", "app", "lpa.h")).read()
    for piece in ("class LabelPropagation", "run(", "labels()", "colors()", "sweeps()", "changes()", "evaluations()", "converged()",
                  "num_communities()", "community_sizes()", "modularity()", "util_symmetrize_simple", "util_lpa_initial_labels"):
        assert piece in lpa_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_lpa.hip" in make and HEADER in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "lpa_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_lpa(None, None, None, None, 1, None) == capi.GL_ERR_NOT_INITIALIZED


def test_closed_forms_of_the_host_truth():
    for k in (3, 17, 65, 130):                            # disjoint cliques: one label each, the second vertex's
        sym, colors, _, _, (label, sweeps, changes, evals, converged) = lpa_case("cliques_%d" % k)
        assert int(colors.max()) + 1 == k
        for i in range(3):
            first = 5 + i * (k + 2)
            assert np.all(label[first:first + k] == first + 1)
        assert (sweeps, changes, converged) == (2, 3 * (k - 1), 1) and evals >= 3 * k
    sym, colors, _, _, (label, sweeps, changes, evals, converged) = lpa_case("star")
    assert colors[7] == 0 and np.all(colors[8:608] == 1)   # the hub takes the smallest leaf, the leaves take the hub's: one label
    assert np.all(label[7:608] == 8) and (sweeps, changes, converged) == (2, 600, 1) and evals == 601 + 1      # sweep 2: the hub alone
    sym, colors, _, _, (label, sweeps, changes, evals, converged) = lpa_case("bipartite")
    used = np.concatenate([np.arange(3, 8), np.arange(20, 27)])
    assert np.unique(label[used]).shape[0] == 1 and converged == 1
    sym, colors, _, _, (label, sweeps, changes, evals, converged) = lpa_case("hubs")
    assert np.unique(label[:302]).shape[0] == 1 and converged == 1
    # a 2-coloured path: the even vertices take their smaller neighbour's label, the odd ones see a tie that includes their own
    sym, colors, _, _, (label, sweeps, changes, evals, converged) = lpa_case("path_2")
    want = np.arange(640)
    want[0:600:2] -= 1
    want[0], want[599] = 1, 597
    assert np.array_equal(label, want) and (sweeps, converged) == (2, 1) and changes == 301
    assert evals == 600 + 1                                # sweep 2: 598 alone, whose neighbour 599 changed behind its evaluation
    for name in COLOR_CASES:                               # isolated vertices are untouched
        sym, colors, init, _, (label, _, _, _, _) = lpa_case(name)
        alone = np.diff(sym.adj_indptr.astype(np.int64)) == 0
        start = np.arange(sym.num_rows) if init is None else init
        assert alone.any() and np.array_equal(label[alone], start[alone])


def test_every_branch_of_the_rule():
    sym, colors, init, after = branches_graph()
    label = lpa_case("branches_1")[4][0]
    assert {c: int(label[c]) for c in after} == after
    assert len(set(init.tolist())) < init.shape[0] and int(init.max()) == TOP
    assert is_fixed_point(sym, lpa_case("branches")[4][0]) and lpa_case("branches")[4][4] == 1


@pytest.mark.parametrize("name", ["path_natural", "cliques_17", "branches", "planted", "planted_seeded"])
def test_every_change_raises_the_edges_whose_ends_share_a_label_and_the_end_is_a_fixed_point(name):
    sym, colors, init, max_sweeps, want = lpa_case(name)
    seen = []

    def on_change(v, old, new, label):
        before = same_label_edges(sym, label)
        label[v] = new
        seen.append(same_label_edges(sym, label) - before)
        label[v] = old
    got = propagate(sym, colors, init, max_sweeps, on_change=on_change)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and want[4] == 1
    assert len(seen) == want[2] and min(seen) >= 1
    assert want[2] <= sym.nnz // 2 and is_fixed_point(sym, want[0])
    start = np.arange(sym.num_rows) if init is None else init
    assert same_label_edges(sym, want[0]) == same_label_edges(sym, start) + sum(seen)


@pytest.mark.parametrize("name", ["path_2", "path_natural", "cliques_65", "hubs", "branches", "planted", "planted_short"])
def test_evaluations_are_the_evaluations_that_saw_a_changed_neighbour(name):
    """a loop that evaluates every vertex with a neighbour in every sweep, and notes which evaluations had a neighbour changed
    since the vertex's previous one: the same labels, sweeps and changes, and that many evaluations"""
    sym, colors, init, max_sweeps, want = lpa_case(name)
    n, hood = sym.num_rows, _hoods(sym)
    label = list(range(n)) if init is None else [int(x) for x in init]
    order = sorted((v for v in range(n) if hood[v]), key=lambda v: (int(colors[v]), v))
    clock, changed_at, seen_at = 0, [0] * n, [-1] * n
    sweeps = changes = needed = 0
    while sweeps < max_sweeps:
        sweeps += 1
        before = changes
        for v in order:
            clock += 1
            if seen_at[v] < 0 or any(changed_at[u] > seen_at[v] for u in hood[v]):
                needed += 1
            else:
                assert _evaluate(label, hood[v], label[v]) == label[v], "evaluating under unchanged neighbour labels changes nothing"
            seen_at[v] = clock
            new = _evaluate(label, hood[v], label[v])
            if new != label[v]:
                label[v], changed_at[v] = new, clock
                changes += 1
        if changes == before:
            break
    assert np.array_equal(np.asarray(label, np.uint32), want[0]) and (sweeps, changes, needed) == want[1:4]
    everything = propagate(sym, colors, init, max_sweeps, use_active=False)
    assert np.array_equal(everything[0], want[0]) and (everything[1], everything[2], everything[4]) == (want[1], want[2], want[4])
    assert everything[3] == len(order) * want[1]


def test_synchronous_schedule_oscillates_where_the_colour_classes_converge():
    for graph in ("bipartite", "path"):
        six, seven = lpa_case("sync_%s_6" % graph)[4], lpa_case("sync_%s_7" % graph)[4]
        assert (six[1], six[4]) == (6, 0) and (seven[1], seven[4]) == (7, 0) and not np.array_equal(six[0], seven[0])
        sym = lpa_case("sync_%s_6" % graph)[0]
        assert propagate(sym, None, None, 40, True)[4] == 0                        # and it goes on
    six, sym = lpa_case("sync_bipartite_6")[4], lpa_case("sync_bipartite_6")[0]
    assert np.array_equal(propagate(sym, None, None, 8, True)[0], six[0])          # K_{5,7} flips with period 2
    label, sweeps, changes, evals, converged = lpa_case("sync_clique_100")[4]
    assert (sweeps, converged) == (3, 1) and np.all(label[5:22] == 5)
    short = lpa_case("planted_short")
    assert short[4][4] == 0 and np.array_equal(short[4][0], lpa_case("planted")[4][0])      # the labels are final a sweep early


@pytest.mark.parametrize("name", COLOR_CASES)
def test_host_truths_agree_on_every_gpu_graph(name):
    sym, colors, init, max_sweeps, want = lpa_case(name)
    start = np.arange(sym.num_rows) if init is None else init
    own = app._lpa_color_loop(sym, colors, start, max_sweeps)
    assert np.array_equal(own[0], want[0]) and own[1:] == want[1:]
    assert app.validate_communities(sym, want[0], colors, init, max_sweeps) == np.unique(want[0]).shape[0]
    best, cur = app._lpa_row_modes(sym, want[0])
    assert bool(np.all(cur == best)) == is_fixed_point(sym, want[0])
    assert want[4] == 0 or is_fixed_point(sym, want[0])


def test_initial_labels_from_a_seed_are_a_permutation():
    a = io.lpa_initial_labels(1000, 3, 1024)
    assert a.dtype == np.uint32 and np.array_equal(np.sort(a[:1000]), np.arange(1000)) and np.array_equal(a[1000:], np.arange(1000, 1024))
    assert not np.array_equal(a, io.lpa_initial_labels(1000, 4, 1024)) and np.array_equal(a, io.lpa_initial_labels(1000, 3, 1024))
    assert np.array_equal(a[:1000], np.argsort(np.argsort(io.coloring_hash(np.arange(1000), 3))))


def test_validate_communities_accepts_the_truth_and_refuses_one_violation_per_rule():
    sym, colors, init, max_sweeps, want = lpa_case("planted")
    label = want[0]
    assert app.validate_communities(sym, label) == app.validate_communities(sym, label, colors) == np.unique(label).shape[0]
    with pytest.raises(ValueError, match="labels for the 1280 vertices"):
        app.validate_communities(sym, label[:100])
    bad = label.copy()
    bad[3] = 5000
    with pytest.raises(ValueError, match=r"vertex 3 carries the label 5000, which no vertex started with \(rule 1\)"):
        app.validate_communities(sym, bad)
    bad = label.copy()
    bad[1250] = label[0]
    with pytest.raises(ValueError, match=r"vertex 1250 has no neighbour and carries %d, not its initial label 1250 \(rule 2\)" % label[0]):
        app.validate_communities(sym, bad)
    other = int(np.flatnonzero(label != label[0])[0])
    bad = label.copy()
    bad[0] = label[other]
    with pytest.raises(ValueError, match=r"neighbours of vertex \d+ carry its label .* not a fixed point \(rule 3\)"):
        app.validate_communities(sym, bad)
    # rule 4: another fixed point -- the same graph swept under another colouring
    shifted = propagate(sym, largest_first(sym, 9), None, 100)[0]
    assert not np.array_equal(shifted, label) and app.validate_communities(sym, shifted) > 0
    with pytest.raises(ValueError, match=r"the loop in \(colour, vertex\) order leaves it \d+ \(rule 4\)"):
        app.validate_communities(sym, shifted, colors)
    short = lpa_case("planted_short")
    assert app.validate_communities(sym, short[4][0], colors, None, short[3]) > 0
    seeded = lpa_case("planted_seeded")
    assert app.validate_communities(sym, seeded[4][0], colors, seeded[2]) > 0
    with pytest.raises(ValueError, match=r"\(rule [14]\)"):
        app.validate_communities(sym, seeded[4][0], colors)


def test_driver_prepares_the_graph_and_refuses_what_it_cannot_do(golden_dir):
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_lpa reads the label"):
        app.LabelPropagation(comm=TwoRanks(), backend=CpuBackend())
    d = app.LabelPropagation(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (d.n_, d.n_real_) == (128, 8) and d.graph_.nnz == 14 and d.degrees_[:8].max() == 2
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        d.modularity()
    # the modularity of two triangles joined by an edge, split at that edge: 6 / 7 - 2 (7 / 14)^2
    a, b = [0, 0, 1, 3, 3, 4, 2], [1, 2, 2, 4, 5, 5, 3]
    d.load_and_format_matrix(raw_csr(128, a, b, np.ones(7)))
    lab = np.arange(128)
    lab[:3], lab[3:6] = 0, 3
    assert abs(d.modularity(lab) - (6.0 / 7.0 - 0.5)) < 1e-12 and abs(d.modularity(np.zeros(128, np.int64))) < 1e-12


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("lpa_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([LPA_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference


def test_walk_stars_the_last_entry_of_every_hub_row_decides():
    """the inputs of tests/test_gpu_walk.py::test_lpa: without the hub's last entry and its mirror every hub with two leaves or
    more ends on another label, under both colourings -- a walk that does not count that entry cannot give the expected labels"""
    from test_gpu_walk import N, _stars, _star_members, lpa_stars, star_hubs
    members, highest = _star_members()
    hubs = star_hubs(2)
    for packed in (False, True):
        sym, colors, init, (lab, sweeps, changes, evals, converged) = lpa_stars(packed)
        assert same_label_edges(sym, colors) == 0 and is_fixed_point(sym, lab)      # a proper colouring
        assert np.array_equal(lab[members], highest) and np.array_equal(np.delete(lab, members), np.delete(np.arange(N), members))
        assert (sweeps, converged) == (2, 1)
        once = propagate(sym, colors, init, 1)[0]
        assert np.array_equal(once, lab)                                 # (sweep 1 decides everything)
        less = lpa_stars(packed, "last")[3][0]
        assert np.all(less[hubs] != lab[hubs]) and np.all(less[hubs] == hubs + 2)      # one of each: the smallest label
