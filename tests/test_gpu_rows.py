"""What a plan knows about its row copy is shared state (csrc/gl_rows.h: rows_sorted, rows_are_sets, rows_symmetric, each
established by whoever asks first): the outcome of every entry point that walks the rows must not depend on which of them touched
the plan first.  Every order below runs on a FRESH boolean plan and calls everything twice -- the second time from the cached
verdicts -- on 256-vertex matrices: accepted calls return the host references' values, refused ones GL_ERR_UNSUPPORTED with the
same message."""
import numpy as np
import pytest

from graphlily_amd import app, capi

from test_cc_cpu import permute_rows
from test_kcore_cpu import _csr
from test_gpu_bc import _bc, _levels
from test_gpu_cc import _labels_of
from test_gpu_kcore import _bool_plan, _clique_edges, _graph, _kcore, _sorted_rows
from test_gpu_tc import _count

pytestmark = pytest.mark.gpu

N, SOURCE = 256, 10
CALLS = ["rows_sorted", "cc_labels", "tc_count", "kcore", "bc_accumulate", "bfs_parents"]
ORDERS = [CALLS[i:] + CALLS[:i] for i in range(len(CALLS))] + [CALLS[::-1]]      # every call first once, and the reversed order


def _matrices():
    a, b = _clique_edges(5, 10)                                                  # K_5 on 10 .. 14, and the edge {20, 21}
    sym = _graph(N, np.concatenate([a, [20]]), np.concatenate([b, [21]]))
    one_way = _sorted_rows(_csr(N, np.concatenate([a, b, [20]]), np.concatenate([b, a, [21]])))      # (20, 21) without (21, 20)
    shuffled = permute_rows(sym, 77)
    assert not np.array_equal(shuffled.adj_indices, sym.adj_indices) and one_way.nnz == sym.nnz - 1
    return {"symmetric": sym, "one_way": one_way, "shuffled": shuffled}


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


def _expected(name, m):
    """call -> the value it must return, or the message fragment it must be refused with"""
    level = _levels(m, None, [SOURCE], N)
    sigma, delta = app.betweenness_by_levels(m, None, level)
    want = {"rows_sorted": name != "shuffled",
            "cc_labels": app._components_of(m.adj_indptr, m.adj_indices, None, N).astype(np.uint32),
            "tc_count": _triangles_by_definition(m),
            "kcore": app._core_numbers_of(m.adj_indptr, m.adj_indices, N).astype(np.uint32),
            "bc_accumulate": (np.where(level >= 2, delta, 0.0), sigma),
            "bfs_parents": _parents_by_definition(m, level)}
    if name == "one_way":
        want["kcore"] = want["bc_accumulate"] = "not symmetric"
    if name == "shuffled":
        want["tc_count"] = want["kcore"] = want["bc_accumulate"] = "strictly ascending"
    return level, want


def _call(plan, call, level):
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
        return _bc(plan, None, level)[:2]
    parent = capi.DeviceBuffer(4 * n)
    plan.bfs_parents(capi.DeviceBuffer.from_host(np.ascontiguousarray(level, np.float32)), parent)
    capi.sync()
    return parent.read(np.uint32, n)


def _same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    return np.array_equal(got, want)


def _run(plan, order, level, want):
    for time in range(2):
        for call in order:
            where = "%s, call %d in the order %s" % (call, time, order)
            if isinstance(want[call], str):
                with pytest.raises(capi.GraphLilyError) as e:
                    _call(plan, call, level)
                assert e.value.code == capi.GL_ERR_UNSUPPORTED and want[call] in str(e.value), where + ": " + str(e.value)
            else:
                assert _same(_call(plan, call, level), want[call]), where


@pytest.mark.parametrize("name", ["symmetric", "one_way", "shuffled"])
def test_outcomes_do_not_depend_on_who_asks_first(gpu, name):
    m = _matrices()[name]
    level, want = _expected(name, m)
    assert want["tc_count"] == "strictly ascending" or want["tc_count"][0] == 60             # K_5: ten triangles, six times each
    for order in ORDERS:
        _run(_bool_plan(m), order, level, want)


def test_a_matrix_without_entries(gpu):
    """it keeps no row copy: the empty graph to gl_tc_count, gl_kcore and gl_bc_accumulate, refused by whoever indexes by row"""
    n = 128
    e = _csr(n, [], [])
    level = np.zeros(n, np.float32)
    level[3] = 1.0
    want = {"rows_sorted": "row copy", "cc_labels": "row copy", "bfs_parents": "row copy", "tc_count": (0, np.zeros(n, np.uint64)),
            "kcore": np.zeros(n, np.uint32), "bc_accumulate": (np.zeros(n), level.astype(np.float64))}
    for order in (CALLS, CALLS[::-1]):
        plan = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
        assert plan.info()["layout"] != "boolean"
        _run(plan, order, level, want)
