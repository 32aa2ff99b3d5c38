"""GPU parity of k-clique counting (gl_clique_count, SpMVPlan.clique_count, app.CliqueCount, graphlily::app::CliqueCount) against
clique_model of tests/test_clique_cpu.py (Python sets, checked there against networkx) and the closed forms of K_n.  Everything
is an integer, so every comparison is np.array_equal.  Every test runs with the default caps, with clique_lds=0 (every matrix
in a global slab) and with clique_tiny=0 clique_mid=0 (every matrix in the wide bin); outputs start as garbage with guard words
behind them, and every check is made twice: the second call runs from the cached bins.  This caller's contract cases (gl_rows.h)
live here."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_kcore_cpu import _csr
from test_clique_cpu import CLIQUE_DRIVER, GOLDEN, clique_model, complete_oriented, row_case

pytestmark = pytest.mark.gpu

G64 = 0xdeadbeefdeadbeef
GUARD = 64
MODES = {"default": {}, "all_in_slabs": {"clique_lds": 0}, "all_wide": {"clique_tiny": 0, "clique_mid": 0}}
ROW_LENGTHS = (2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


@pytest.fixture(autouse=True, params=sorted(MODES))
def mode(request, monkeypatch):
    for key, value in MODES[request.param].items():
        set_knob(monkeypatch, key, value)
    return request.param


def _bool_plan(m, r0=0, r1=None):
    return capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)


def _count(plan, n, k, per_vertex=True):
    """-> (total, per or None, stats); the guard words behind both outputs must still be garbage"""
    total = capi.DeviceBuffer.from_host(np.full(1 + GUARD, G64, np.uint64))
    per = capi.DeviceBuffer.from_host(np.full(n + GUARD, G64, np.uint64)) if per_vertex else None
    stats = plan.clique_count(k, total, per, stats=True)
    capi.sync()
    t = total.read(np.uint64, 1 + GUARD)
    assert np.all(t[1:] == G64), "a guard word behind the total was written"
    p = None
    if per_vertex:
        p = per.read(np.uint64, n + GUARD)
        assert np.all(p[n:] == G64), "a guard word behind the per-vertex counts was written"
        p = p[:n]
    assert len(stats) == 4 and G64 not in stats
    return int(t[0]), p, stats


def _check(csr, k, want, plan=None, what=""):
    plan = _bool_plan(csr) if plan is None else plan
    for call in range(2):
        total, per, stats = _count(plan, csr.num_rows, k)
        assert total == want[0], (what, k, call, total, want[0])
        assert np.array_equal(per, want[1]), "%s k=%d call %d: first difference at vertex %d" % (what, k, call, int(np.flatnonzero(per != want[1])[0]))
        assert _count(plan, csr.num_rows, k, per_vertex=False)[0] == want[0], (what, k, call, "total only")
    return stats


@functools.lru_cache(maxsize=None)
def _row_model(d, k):
    return clique_model(row_case(d)[0], k)


@pytest.mark.parametrize("d", ROW_LENGTHS)
def test_a_row_of_exactly_d_entries(gpu, mode, d):
    csr, _ = row_case(d)
    plan = _bool_plan(csr)
    for k in range(3, 9 if d <= 65 else 7):
        want = _row_model(d, k)
        assert d < k - 1 or k > min(7, d) + 1 or want[0] > 0
        stats = _check(csr, k, want, plan, "d=%d" % d)
    rows = np.diff(csr.adj_indptr.astype(np.int64))
    binned = int(np.count_nonzero(rows >= 2))
    if mode == "all_in_slabs":
        assert stats[:3] == (0, 0, binned)
    elif mode == "all_wide":
        assert stats[:3] == (0, int(np.count_nonzero((rows >= 2) & (rows <= 1024))), int(np.count_nonzero(rows > 1024)))
    else:
        assert stats[:3] == (int(np.count_nonzero((rows >= 2) & (rows <= 256))), int(np.count_nonzero((rows > 256) & (rows <= 1024))),
                             int(np.count_nonzero(rows > 1024)))


@pytest.mark.parametrize("n", [4, 33, 65, 257, 1025])
def test_complete_graphs_have_closed_forms(gpu, n):
    csr = complete_oriented(n)
    plan = _bool_plan(csr)
    for k in range(3, 5 if n == 1025 else 6):
        _check(csr, k, (math.comb(n, k), np.full(n, math.comb(n - 1, k - 1), np.uint64)), plan, "K_%d" % n)


def test_edge_inputs(gpu):
    n = 128
    empty = io.CSRMatrix(n, n, np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(n + 1, np.uint32))
    assert _check(empty, 4, (0, np.zeros(n, np.uint64)), what="no entries") == (0, 0, 0, 0)
    short = row_case(3)[0]                                                  # rows shorter than k - 1
    _check(short, 6, (0, np.zeros(short.num_rows, np.uint64)), what="short rows")
    sym, _ = io.symmetrize_simple(row_case(33)[0])                          # unoriented: every clique in every order
    for k in (3, 4, 5):
        total, per = _row_model(33, k)
        _check(sym, k, (math.factorial(k) * total, math.factorial(k) * per), what="symmetric")
    rng = np.random.default_rng(8)
    rows, cols = rng.integers(0, 40, 300), rng.integers(0, 40, 300)
    loops = np.arange(0, 40, 3)                                             # diagonal entries take part; rows of one entry count
    key = np.unique(np.concatenate([rows, loops, [40]]) * 41 + np.concatenate([cols, loops, [0]]))    # rows as ascending sets
    diag = _csr(41, key // 41, key % 41)
    for k in (3, 4, 5):
        _check(diag, k, clique_model(diag, k), what="diagonal")


@pytest.mark.parametrize("d", [33, 1025])
def test_k3_is_tc_count_to_the_bit(gpu, d):
    csr, _ = row_case(d)
    plan = _bool_plan(csr)
    n = csr.num_rows
    total, per = capi.DeviceBuffer.from_host(np.full(1, G64, np.uint64)), capi.DeviceBuffer.from_host(np.full(n, G64, np.uint64))
    plan.tc_count(total, per)
    capi.sync()
    _check(csr, 3, (int(total.read(np.uint64, 1)[0]), per.read(np.uint64, n)), plan, "tc")


def test_error_paths(gpu, monkeypatch):
    csr, _ = row_case(33)
    n = csr.num_rows
    plan = _bool_plan(csr)
    total = capi.DeviceBuffer.from_host(np.full(1, G64, np.uint64))
    for k in (2, 9):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.clique_count(k, total)
        assert e.value.code == capi.GL_ERR_INVALID_ARG and "gl_clique_count" in str(e.value), str(e.value)
    with pytest.raises(capi.GraphLilyError) as e:
        plan.clique_count(3, None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG

    def refused(p, *needles):
        for _ in range(2):
            with pytest.raises(capi.GraphLilyError) as e:
                p.clique_count(4, total)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and "gl_clique_count" in str(e.value), str(e.value)
            for needle in needles:
                assert needle in str(e.value), str(e.value)
        capi.sync()
        assert int(total.read(np.uint64, 1)[0]) == G64

    m = 8200
    refused(_bool_plan(_csr(m, np.zeros(8193, np.int64), np.arange(1, 8194))), "8193 entries", "io.orient_by_rank", "KCore.run(order=True)")
    set_knob(monkeypatch, "clique_scratch_mb", 0)
    refused(_bool_plan(row_case(1025)[0]), "clique_scratch_mb", "io.orient_by_rank")
    set_knob(monkeypatch, "clique_scratch_mb", None)
    refused(_bool_plan(csr, 0, n // 2), "row shard")
    refused(_bool_plan(io.CSRMatrix(n, n + 128, csr.adj_data, csr.adj_indices, csr.adj_indptr)), "num_rows == num_cols")
    unsorted = csr.adj_indices.copy()
    unsorted[:33] = unsorted[:33][::-1]
    refused(_bool_plan(io.CSRMatrix(n, n, csr.adj_data, unsorted, csr.adj_indptr)), "strictly ascending sets", "io.orient_by_rank")


def _driver(path, rank=None):
    d = app.CliqueCount(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(path, rank)
    d.send_matrix_host_to_device()
    return d


def test_drivers_on_the_golden_file(gpu, golden_dir, tmp_path):
    path = os.path.join(golden_dir, GOLDEN)
    raw = io.load_csr_matrix_from_float_npz(path)
    d = _driver(path)
    kc = app.KCore(M.num_hbm_channels, 1024, 256)
    kc.set_target("hw")
    kc.set_up_runtime("unused.xclbin")
    kc.load_and_format_matrix(path, True)
    kc.send_matrix_host_to_device()
    kc.run(order=True)
    position = np.empty(kc.n_, dtype=np.uint32)
    position[kc.order_] = np.arange(kc.n_, dtype=np.uint32)
    by_degeneracy = _driver(path, position)
    padded = io.load_csr_matrix_from_float_npz(path)
    io.util_round_csr_matrix_dim(padded, d.n_, d.n_)
    assert kc.n_ == d.n_ == padded.num_rows
    assert np.diff(io.orient_by_rank(padded, position)[0].adj_indptr.astype(np.int64)).max() <= kc.degeneracy_    # the recipe's point
    for k in (3, 4, 5):
        cliques = d.run(k)
        want = clique_model(io.orient_by_rank(padded)[0], k)
        assert cliques.dtype == np.uint64 and np.array_equal(cliques, want[1]) and d.num_cliques_ == want[0] and d.k_ == k
        assert app.validate_cliques(raw, k, cliques) == d.num_cliques_ > 0
        assert d.clique_density() == d.num_cliques_ / math.comb(d.n_real_, k) and len(d.bins_) == 4
        assert d.run(k, per_vertex=False) == want[0] and d.cliques_ is None
        assert np.array_equal(by_degeneracy.run(k), cliques) and by_degeneracy.num_cliques_ == want[0]
        r = subprocess.run([CLIQUE_DRIVER, path, str(tmp_path), str(k)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "CliqueCount::run OK" in r.stdout and "cliques: %d\n" % want[0] in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
        assert np.array_equal(np.fromfile(os.path.join(str(tmp_path), "cpp_cliques.bin"), dtype=np.uint64), cliques)
