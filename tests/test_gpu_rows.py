"""What a plan knows about its row copy is shared state (csrc/gl_rows.h: rows_sorted, rows_are_sets, rows_symmetric, each
established by whoever asks first, and the transpose partner that rows_require_pair caches): the outcome of every entry point
that walks the rows must not depend on which of them touched the plan first.  The entry points: rows_sorted, gl_cc_labels and
gl_bfs_parents (kRowsIndexable), gl_tc_count (kRowsSets), gl_kcore, gl_color, gl_msf, gl_truss, gl_match, gl_lpa and
gl_louvain_move (kRowsSymmetric), gl_bc_accumulate and gl_scc (rows_require_pair; with one plan: kRowsSymmetric).  Every order
below runs on a FRESH boolean plan and calls everything twice -- the second time from the cached verdicts -- on 256-vertex
matrices: accepted calls return the host references' values, refused ones GL_ERR_UNSUPPORTED with the same message."""
import numpy as np
import pytest

from graphlily_amd import app, capi, io

from test_cc_cpu import permute_rows
from test_coloring_cpu import greedy_by_priority
from test_kcore_cpu import _csr
from test_gpu_bc import _bc, _levels
from test_gpu_cc import _labels_of
from test_gpu_coloring import _color
from test_gpu_kcore import _bool_plan, _clique_edges, _graph, _kcore, _sorted_rows
from test_gpu_louvain import _move
from test_gpu_lpa import _lpa
from test_gpu_match import _match
from test_gpu_msf import _msf
from test_gpu_scc import _scc
from test_gpu_tc import _count
from test_gpu_truss import _truss
from test_louvain_cpu import move_loop
from test_lpa_cpu import greedy_colors, propagate
from test_match_cpu import FREE, greedy, pairs_of, pointer_rounds
from test_msf_cpu import kruskal
from test_scc_cpu import scc_model
from test_truss_cpu import truss_numbers

pytestmark = pytest.mark.gpu

N, SOURCE, SWEEPS = 256, 10, 10
GARBAGE = 0xdeadbeef
CALLS = ["rows_sorted", "cc_labels", "tc_count", "kcore", "bc_accumulate", "bfs_parents",
         "color", "msf", "truss", "match", "lpa", "louvain_move", "scc"]
SYMMETRIC_ONLY = ["kcore", "bc_accumulate", "color", "msf", "truss", "match", "lpa", "louvain_move", "scc"]      # kRowsSymmetric
ORDERS = [CALLS[i:] + CALLS[:i] for i in range(len(CALLS))] + [CALLS[::-1]]      # every call first once and last once, and the reversed order


def _matrices():
    a, b = _clique_edges(5, 10)                                                  # K_5 on 10 .. 14, and the edge {20, 21}
    sym = _graph(N, np.concatenate([a, [20]]), np.concatenate([b, [21]]))
    one_way = _sorted_rows(_csr(N, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]])))      # (20, 21) without (21, 20)
    shuffled = permute_rows(sym, 77)
    assert not np.array_equal(shuffled.adj_indices, sym.adj_indices) and one_way.nnz == sym.nnz - 1
    return {"symmetric": sym, "one_way": one_way, "shuffled": shuffled}


def _entries(m):
    return np.repeat(np.arange(m.num_rows, dtype=np.int64), np.diff(m.adj_indptr.astype(np.int64))), m.adj_indices.astype(np.int64)


def _weights(m):
    """a distinct whole weight per edge, the same in (v, u) and (u, v) (exact in f32)"""
    rows, cols = _entries(m)
    return (1 + np.minimum(rows, cols) * N + np.maximum(rows, cols)).astype(np.float32)


def _triangles_by_definition(m):
    """(sum over v, u in N(v) of |N(v) & N(u)|, the credits of every vertex) over the rows as sets"""
    ip = m.adj_indptr.astype(np.int64)
    rows = [set(int(c) for c in m.adj_indices[ip[v]:ip[v + 1]]) for v in range(m.num_rows)]
    per = np.zeros(m.num_rows, np.uint64)
    for v, nv in enumerate(rows):
        for u in nv:
            for w in nv & rows[u]:
                per[[v, u, w]] += np.uint64(1)
    return int(per.sum()) // 3, per


def _parents_by_definition(m, level):
    ip = m.adj_indptr.astype(np.int64)
    out = np.full(m.num_rows, 0xffffffff, np.uint32)
    for v in range(m.num_rows):
        row = m.adj_indices[ip[v]:ip[v + 1]]
        hits = row[level[row] == level[v] - 1]
        out[v] = v if level[v] == 1 else hits.min() if level[v] >= 2 and hits.size else 0xffffffff
    return out


def _scc_expected(m):
    """(labels, (components, passes, trimmed)) of scc_model on the edges u -> v of the entries A[v, u]"""
    rows, cols = _entries(m)
    lab, comps, passes, trimmed, _ = scc_model(m.num_rows, cols, rows)
    return lab, (comps, passes, trimmed)


def _symmetric_expected(m, inputs):
    """the seven callers that only a symmetric matrix reaches, from their suites' host models"""
    weighted = io.CSRMatrix(N, N, inputs["weights"], m.adj_indices, m.adj_indptr)
    mate, rounds, scans = pointer_rounds(weighted)
    assert np.array_equal(mate, greedy(weighted))
    truss, support, _, sub_rounds, triangles = truss_numbers(m)
    lab, sweeps, changes, evals, converged = propagate(m, inputs["colors"], None, SWEEPS)
    moved = move_loop(m, None, None, inputs["colors"], SWEEPS, 0)
    return {"color": greedy_by_priority(m, None)[0],
            "msf": (kruskal(weighted).astype(np.uint32), app._components_of(m.adj_indptr, m.adj_indices, None, N).astype(np.uint32),
                    (5, N - 5)),
            "truss": (truss, support, (int(truss.max()), int(np.unique(truss[truss > 0]).shape[0]), sub_rounds, m.nnz // 2, triangles)),
            "match": (mate, (len(pairs_of(mate)), rounds, scans)),
            "lpa": (lab, (sweeps, changes, evals, converged)),
            "louvain_move": (moved[0], tuple(moved[1:])),
            "scc": _scc_expected(m)}


def _expected(name, m):
    """call -> the value it must return, or the message fragment it must be refused with; and what the calls take beside the plan"""
    level = _levels(m, None, [SOURCE], N)
    inputs = {"level": level, "weights": _weights(m), "colors": greedy_colors(_matrices()["symmetric"]), "nnz": m.nnz}
    sigma, delta = app.betweenness_by_levels(m, None, level)
    want = {"rows_sorted": name != "shuffled",
            "cc_labels": app._components_of(m.adj_indptr, m.adj_indices, None, N).astype(np.uint32),
            "tc_count": _triangles_by_definition(m),
            "kcore": app._core_numbers_of(m.adj_indptr, m.adj_indices, N).astype(np.uint32),
            "bc_accumulate": (np.where(level >= 2, delta, 0.0), sigma),
            "bfs_parents": _parents_by_definition(m, level)}
    if name == "symmetric":
        want.update(_symmetric_expected(m, inputs))
    # the refusals, in rows_require's order: the sets before the symmetry, and gl_tc_count asks for the sets only
    if name == "one_way":
        want.update({call: "not symmetric" for call in SYMMETRIC_ONLY})
    if name == "shuffled":
        want.update({call: "strictly ascending" for call in SYMMETRIC_ONLY + ["tc_count"]})
    assert sorted(want) == sorted(CALLS)
    return inputs, want


def _call(plan, call, inputs, plan_out=None):
    """(plan_out: for the two calls that take a second plan; None declares the pattern symmetric)"""
    level = inputs["level"]
    n = level.shape[0]
    if call == "rows_sorted":
        return plan.rows_sorted()
    if call == "cc_labels":
        return _labels_of(plan, n, with_count=False)[0]
    if call == "tc_count":
        return _count(plan, n)
    if call == "kcore":
        return _kcore(plan, n, order=False)[0]
    if call == "bc_accumulate":
        return _bc(plan, plan_out, level)[:2]
    if call == "color":
        return _color(plan, n)[0]
    if call == "msf":
        forest, labels, stats = _msf(plan, inputs["weights"], n)
        return forest, labels, stats[:2]
    if call == "truss":
        truss, support, stats = _truss(plan, inputs["nnz"])
        return truss, support, stats[:3] + stats[4:]
    if call == "match":
        mate, stats = _match(plan, inputs["weights"], n)
        return mate, stats[:3]
    if call == "lpa":
        label, stats = _lpa(plan, n, inputs["colors"], None, SWEEPS)
        return label, (stats[0], stats[1], stats[2], stats[4])
    if call == "louvain_move":
        label, stats = _move(plan, n, None, None, inputs["colors"], SWEEPS, 0)
        return label, stats[:3] + stats[4:]
    if call == "scc":
        label, stats = _scc(plan, plan_out, n)
        return label, stats[:3]
    parent = capi.DeviceBuffer(4 * n)
    plan.bfs_parents(capi.DeviceBuffer.from_host(np.ascontiguousarray(level, np.float32)), parent)
    capi.sync()
    return parent.read(np.uint32, n)


def _same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    return np.array_equal(got, want)


def _refused(fragment, where, call, *args):
    with pytest.raises(capi.GraphLilyError) as e:
        call(*args)
    assert e.value.code == capi.GL_ERR_UNSUPPORTED and fragment in str(e.value), where + ": " + str(e.value)


def _run(plan, order, inputs, want):
    for time in range(2):
        for call in order:
            where = "%s, call %d in the order %s" % (call, time, order)
            if isinstance(want[call], str):
                _refused(want[call], where, _call, plan, call, inputs)
            else:
                assert _same(_call(plan, call, inputs), want[call]), where


@pytest.mark.parametrize("name", ["symmetric", "one_way", "shuffled"])
def test_outcomes_do_not_depend_on_who_asks_first(gpu, name):
    m = _matrices()[name]
    inputs, want = _expected(name, m)
    assert want["tc_count"] == "strictly ascending" or want["tc_count"][0] == 60             # K_5: ten triangles, six times each
    if name == "symmetric":                                  # the closed forms, so that no comparison is between two empty answers
        assert int(want["color"].max()) == 4 and int(want["msf"][0].sum()) == 2 * 5 and want["truss"][2][:2] + want["truss"][2][3:] == (5, 2, 11, 10)
        assert want["match"][1][0] == 3 and want["scc"][1] == (1 + 1 + 249, 1, 249)
        assert np.unique(want["lpa"][0][10:15]).shape[0] == 1 == np.unique(want["louvain_move"][0][10:15]).shape[0]
        assert want["lpa"][1][3] == 1 and want["louvain_move"][1][3] == 1 and want["louvain_move"][1][5] > want["louvain_move"][1][4]
    for order in ORDERS:
        _run(_bool_plan(m), order, inputs, want)


def test_the_transpose_partner_is_cached_per_handle(gpu):
    """gl_scc and gl_bc_accumulate with TWO plans, the one-way matrix and its transpose: whoever asks first establishes plan_in's
    partner verdict and the other reuses it; a plan_out that is NOT the transpose -- with one entry more, and with as many -- is
    refused although the right partner's verdict is cached, and the right one is accepted again behind the wrong ones"""
    cin = _matrices()["one_way"]
    rows, cols = _entries(cin)
    cout = _sorted_rows(_csr(N, cols, rows))
    level = _levels(cin, cout, [SOURCE], N)
    inputs = {"level": level}
    sigma, delta = app.betweenness_by_levels(cin, cout, level)
    want = {"scc": _scc_expected(cin), "bc_accumulate": (np.where(level >= 2, delta, 0.0), sigma)}
    assert want["scc"][1] == (1 + 251, 1, 251) and np.count_nonzero(want["bc_accumulate"][1]) == 5      # (20 -> 21 is no cycle)
    for order in (["scc", "bc_accumulate"], ["bc_accumulate", "scc"]):
        pin, pout = _bool_plan(cin), _bool_plan(cout)
        wrong = [_bool_plan(_matrices()["symmetric"]), _bool_plan(cin)]          # the missing (21, 20) too; plan_in's own pattern
        for time in range(2):
            for call in order:
                where = "%s, call %d in the order %s" % (call, time, order)
                assert _same(_call(pin, call, inputs, pout), want[call]), where
        for other in wrong + wrong[::-1]:
            for call in order:
                for time in range(2):
                    _refused("not the transpose", "%s with another plan_out" % call, _call, pin, call, inputs, other)
                assert _same(_call(pin, call, inputs, pout), want[call]), call + " with the right partner again"
        for call in order:                                                      # ... and one plan for both is the symmetric declaration
            _refused("not symmetric", call, _call, pin, call, inputs, None)
            assert _same(_call(pin, call, inputs, pout), want[call]), call


def test_a_matrix_without_entries(gpu):
    """it keeps no row copy: the empty graph to everybody who asks for a square matrix -- each answers as its own suite's test of a
    plan without entries says --, refused by whoever indexes by row"""
    n = 128
    e = _csr(n, [], [])
    level = np.zeros(n, np.float32)
    level[3] = 1.0
    inputs = {"level": level, "weights": np.zeros(16, np.float32), "colors": np.zeros(n, np.uint32), "nnz": 16}
    iota, untouched = np.arange(n, dtype=np.uint32), np.full(16, GARBAGE, np.uint32)
    want = {"rows_sorted": "row copy", "cc_labels": "row copy", "bfs_parents": "row copy", "tc_count": (0, np.zeros(n, np.uint64)),
            "kcore": np.zeros(n, np.uint32), "bc_accumulate": (np.zeros(n), level.astype(np.float64)),
            "color": np.zeros(n, np.uint32), "msf": (untouched, iota, (0, n)), "truss": (untouched, untouched, (0, 0, 0, 0, 0)),
            "match": (np.full(n, FREE, np.uint32), (0, 0, 0)), "lpa": (iota, (1, 0, 0, 1)), "louvain_move": (iota, (1, 0, 0, 1, 0, 0)),
            "scc": (iota, (n, 0, 0))}
    assert sorted(want) == sorted(CALLS)
    for order in (CALLS, CALLS[::-1]):
        plan = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
        assert plan.info()["layout"] != "boolean"
        _run(plan, order, inputs, want)
