"""GPU parity of the triangle counting (gl_tc_count, SpMVPlan.tc_count, SpMVModule.tc_count, app.TriangleCount,
graphlily::app::TriangleCount): every comparison is np.array_equal / == against the scipy statement of the definition
(tests/test_tc_cpu.py) or a closed form.  The definition is exact: no tolerance anywhere."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver, named_matrix, set_knob
from test_cc_cpu import many_components, permute_rows
from test_tc_cpu import (MANY_CYCLES, ROOT, TC_DRIVER, _csr, _from_scipy, abi_counts, symmetric_simple,
                         triangles_by_definition)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["line_8", "eye_10"]
# triangles, counted on the CPU (scipy, the symmetrised pattern)
TOTALS = {"uniform_10K_10": 1151, "rmat_20K": 6312502, "rmat_sym_50K": 11501410, "gplus_small": 69029364, "line_8": 0, "eye_10": 0,
          "many": MANY_CYCLES[3]}
PER_VERTEX = ["uniform_10K_10", "rmat_20K", "line_8", "eye_10", "many"]     # where the host reference takes a second or two
# the LDS budget of gl_tc.hip: a wavefront's slice holds at most tc_lds = 4096 entries of a row (kTcMaxLds: 16 KiB); a longer row
# is searched in global memory.  Rows of 33 .. 1024 entries share a workgroup four wavefronts at a time, longer ones have one each.
LDS_BUDGET = 4096


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """-> (the matrix as given, padded to 128, triangles through every vertex of the padded matrix or None, undirected
    degrees); computed once and shared, never written"""
    if name in FIXTURES:
        raw = io.load_csr_matrix_from_float_npz(os.path.join(GOLDEN, name + "_csr_float32.npz"))
    elif name == "many":
        raw = many_components()
    else:
        raw = named_matrix(name)
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    t = None
    deg = np.asarray(symmetric_simple(m).sum(axis=1)).ravel().astype(np.int64)      # (no sparse product: cheap on every graph)
    if name in PER_VERTEX:
        t, deg2 = triangles_by_definition(m)
        t.setflags(write=False)
        assert int(t.sum()) == 3 * TOTALS[name] and np.array_equal(deg, deg2)
    return raw, m, t, deg


def _driver(m):
    tc = app.TriangleCount(M.num_hbm_channels, 1024, 256)
    tc.set_target("hw")
    tc.set_up_runtime("unused.xclbin")
    tc.load_and_format_matrix(m, True)
    tc.send_matrix_host_to_device()
    return tc


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _count(plan, n, per_vertex=True):
    """-> (total, per-vertex counts or None); both buffers start out as garbage: the call zeroes them itself"""
    total = capi.DeviceBuffer.from_host(np.array([0xdeadbeefdeadbeef], np.uint64))
    per = capi.DeviceBuffer.from_host(np.full(n, 12345, np.uint64)) if per_vertex else None
    plan.tc_count(total, per)
    capi.sync()
    return int(total.read(np.uint64, 1)[0]), (per.read(np.uint64, n) if per_vertex else None)


@pytest.mark.parametrize("name", ["uniform_10K_10", "rmat_20K", "rmat_sym_50K", "gplus_small"] + FIXTURES + ["many"])
def test_drivers(gpu, name):
    raw, m, want, deg = _prepared(name)
    tc = _driver(raw)
    got = tc.run()
    assert got.dtype == np.uint64 and got.shape == (m.num_rows,) and tc.n_real_ == raw.num_rows
    assert tc.num_triangles_ == TOTALS[name] and int(got.sum()) == 3 * TOTALS[name] and tc.triangles_ is got
    assert not got[raw.num_rows:].any()
    assert np.array_equal(tc.degrees_, deg)
    wedges = sum(int(d) * (int(d) - 1) // 2 for d in deg)
    assert type(tc.num_wedges_) is int and tc.num_wedges_ == wedges
    assert tc.transitivity_ == (3.0 * TOTALS[name] / wedges if wedges else 0.0)
    if want is not None:
        assert np.array_equal(got, want)
        assert app.validate_triangles(m, got) == TOTALS[name]
        c = tc.clustering()
        pairs = deg.astype(np.float64) * (deg.astype(np.float64) - 1.0)
        assert np.array_equal(c, np.divide(2.0 * want.astype(np.float64), pairs, out=np.zeros(m.num_rows), where=pairs > 0))
    assert np.array_equal(tc.run(), got)                                     # a second run, on the cached verdict and bins
    assert tc.run(per_vertex=False) == TOTALS[name] and tc.triangles_ is None and tc.num_triangles_ == TOTALS[name]


def _clique(k, n, full=False):
    iu = np.triu_indices(k, 1)
    rows, cols = (np.concatenate(iu), np.concatenate(iu[::-1])) if full else iu
    return _csr(n, rows + 5, cols + 5)           # (the clique sits on vertices 5 .. k + 4)


@pytest.mark.parametrize("k", [3, 4, 63, 64, 65, 66, 129])
def test_cliques_across_the_row_length_boundaries(gpu, k):
    """K_k as an upper triangle: row lengths k - 1 .. 0, across the sub-wave group (16), the short bin (32) and the wavefront (64)"""
    n = 256
    want = np.zeros(n, np.uint64)
    want[5:5 + k] = math.comb(k - 1, 2)
    total, per = _count(_bool_plan(_clique(k, n)), n)
    assert total == math.comb(k, 3) and np.array_equal(per, want)
    plan = _bool_plan(_clique(k, n, full=True))
    total, per = _count(plan, n)
    assert total == 6 * math.comb(k, 3) and np.array_equal(per, 6 * want)
    assert _count(plan, n, per_vertex=False) == (6 * math.comb(k, 3), None)


def test_diagonal_empty_and_single_edge(gpu):
    n = 128
    rng = np.random.default_rng(17)
    rows, cols = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    key = np.unique(np.concatenate([rows * n + cols, np.arange(0, n, 3) * (n + 1)]))      # a set per row, a third of the diagonal
    d = _csr(n, key // n, key % n)
    assert np.count_nonzero((key // n) == (key % n)) >= n // 3
    want_total, want_per = abi_counts(d)
    assert _count(_bool_plan(d), n) [0] == want_total
    assert np.array_equal(_count(_bool_plan(d), n)[1], want_per)
    tiny = _csr(n, [0, 0, 1], [0, 1, 1])         # N(0) = {0, 1}, N(1) = {1}: the triples (0,0,0), (0,0,1), (0,1,1), (1,1,1)
    total, per = _count(_bool_plan(tiny), n)
    assert total == 4 and per[0] == 6 and per[1] == 6 and not per[2:].any()
    e = _csr(n, [], [])                          # (a matrix without entries is planned in the general layout whatever the flags)
    empty = capi.SpMVPlan(n, n, e.adj_indptr, e.adj_indices, e.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        total, per = _count(empty, n)
        assert total == 0 and not per.any()
    assert _count(empty, n, per_vertex=False) == (0, None)
    total, per = _count(_bool_plan(_csr(n, [3], [100])), n)
    assert total == 0 and not per.any()


@pytest.mark.parametrize("knob,value", [("tc_group", 8), ("tc_group", 32), ("tc_group", 64), ("tc_search", 1)])
def test_group_sizes_and_the_flipped_search(gpu, monkeypatch, knob, value):
    """the other instantiations of the short bin, and the search of N(v)'s entries in a longer N(u) (tc_search=1; tc_flip=1 turns
    every pair with a longer N(u) round, the default 8 only the lopsided ones): the knobs are read per call"""
    _, padded, t, _ = _prepared("rmat_20K")
    o, _ = io.triangle_orient(padded)
    n = o.num_rows
    sym = _from_scipy(symmetric_simple(padded))                 # (un-oriented: short rows next to hubs, so pairs are lopsided)
    plans = [(_bool_plan(o), 1), (_bool_plan(sym), 6)]
    for flip in ((None, 1) if knob == "tc_search" else (None,)):
        set_knob(monkeypatch, knob, value)
        set_knob(monkeypatch, "tc_flip", flip)
        for plan, times in plans:
            total, per = _count(plan, n)
            assert total == times * TOTALS["rmat_20K"] and np.array_equal(per, times * t)
            assert _count(plan, n, per_vertex=False)[0] == times * TOTALS["rmat_20K"]
    k = 66                                                      # row lengths 65 .. 0: every bin boundary of every group size
    want = np.zeros(256, np.uint64)
    want[5:5 + k] = math.comb(k - 1, 2)
    total, per = _count(_bool_plan(_clique(k, 256)), 256)
    assert total == math.comb(k, 3) and np.array_equal(per, want)


def test_entry_list_with_a_nonzero_first_offset(gpu):
    """the C ABI accepts a whole-matrix CSR whose indptr[0] is k != 0: the row copy's offsets then count from the caller's entry
    list while its indices start at entry k (csr_nz_base)"""
    _, padded, t, _ = _prepared("uniform_10K_10")
    o, _ = io.triangle_orient(padded)
    n, k = o.num_rows, 77
    junk = np.full(k, n - 1, np.uint32)                         # (entries in front of row 0 that belong to no row)
    plan = capi.SpMVPlan(n, n, o.adj_indptr + np.uint32(k), np.concatenate([junk, o.adj_indices]),
                         np.concatenate([np.ones(k, np.float32), o.adj_data]), 0, n, flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean" and plan.info()["nnz"] == o.nnz
    for _ in range(2):
        total, per = _count(plan, n)
        assert total == TOTALS["uniform_10K_10"] and np.array_equal(per, t)
    # K_200's rows run through the short and wave bins, the star's row of 5000 entries through the chunks of the long bin
    iu = np.triu_indices(200, 1)
    m = _csr(5120, np.concatenate([np.zeros(5000, np.int64), iu[0] + 1]), np.concatenate([np.arange(1, 5001), iu[1] + 1]))
    want_total, want_per = abi_counts(m)
    plan = capi.SpMVPlan(5120, 5120, m.adj_indptr + np.uint32(k), np.concatenate([junk[:k] * 0, m.adj_indices]),
                         np.concatenate([np.ones(k, np.float32), m.adj_data]), 0, 5120, flags=capi.GL_PLAN_BOOLEAN)
    total, per = _count(plan, 5120)
    assert np.diff(m.adj_indptr.astype(np.int64)).max() == 5000 > LDS_BUDGET
    assert total == want_total == math.comb(200, 2) + math.comb(200, 3) and np.array_equal(per, want_per)


def test_total_above_32_bits(gpu):
    """K_3000 as an upper triangle: C(3000, 3) = 4 495 501 000 > 2^32; its rows run through the short, wave and wide bins"""
    k, n = 3000, 3072
    iu = np.triu_indices(k, 1)
    total, per = _count(_bool_plan(_csr(n, iu[0], iu[1])), n)
    assert total == 4_495_501_000 == math.comb(k, 3) and total > 1 << 32
    want = np.zeros(n, np.uint64)
    want[:k] = math.comb(k - 1, 2)
    assert np.array_equal(per, want)


def test_rows_longer_than_the_lds_budget(gpu):
    """the global-memory path: a star of 100 000 leaves around vertex 0 plus K_20 on the vertices 1 .. 20, stored one way; and the
    symmetric rmat_20K as it is, un-oriented, whose longest row has 5133 entries"""
    leaves, n = 100000, 100096
    iu = np.triu_indices(20, 1)
    m = _csr(n, np.concatenate([np.zeros(leaves, np.int64), iu[0] + 1]), np.concatenate([np.arange(1, leaves + 1), iu[1] + 1]))
    assert np.diff(m.adj_indptr.astype(np.int64)).max() == leaves > LDS_BUDGET
    want_total, want_per = abi_counts(m)
    assert want_total == math.comb(20, 2) + math.comb(20, 3)        # row 0 meets every row of the clique in that row itself
    plan = _bool_plan(m)
    total, per = _count(plan, n)
    assert total == want_total and np.array_equal(per, want_per)
    assert _count(plan, n, per_vertex=False)[0] == want_total
    _, padded, t, deg = _prepared("rmat_20K")
    sym = _from_scipy(symmetric_simple(padded))
    lens = np.diff(sym.adj_indptr.astype(np.int64))
    assert lens.max() == 5133 > LDS_BUDGET and np.count_nonzero(lens > 1024) == 70
    total, per = _count(_bool_plan(sym), sym.num_rows)
    assert total == 6 * TOTALS["rmat_20K"] and np.array_equal(per, 6 * t)


def test_refusals(gpu):
    _, padded, t, _ = _prepared("uniform_10K_10")
    good, _ = io.triangle_orient(padded)
    n = good.num_rows
    plan = _bool_plan(good)

    def still_works():
        total, per = _count(plan, n)
        assert total == TOTALS["uniform_10K_10"] and np.array_equal(per, t)
    still_works()
    assert _count(plan, n, per_vertex=False) == (TOTALS["uniform_10K_10"], None)          # d_per_vertex may be NULL
    total = capi.DeviceBuffer(8)

    def refused(p, needle):
        for _ in range(2):                                                  # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.tc_count(total)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
        still_works()
    general = capi.SpMVPlan(good.num_rows, good.num_cols, good.adj_indptr, good.adj_indices, good.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "row copy")
    refused(_bool_plan(good, 0, n // 2), "row shard")
    refused(_bool_plan(good, n // 2, n), "row shard")
    sym = _from_scipy(symmetric_simple(padded))                             # (rows long enough for a shuffle to show)
    assert _count(_bool_plan(sym), n)[0] == 6 * TOTALS["uniform_10K_10"]
    sh = permute_rows(sym, 77)
    assert not np.array_equal(sh.adj_indices, sym.adj_indices)
    refused(_bool_plan(sh), "io.triangle_orient")
    z = good.copy()
    z.adj_data[np.random.default_rng(2).random(z.nnz) < 0.01] = 0.0
    assert np.any(z.adj_data == 0)
    refused(_bool_plan(z), "io.triangle_orient")
    ip = good.adj_indptr.astype(np.int64)
    r = int(np.flatnonzero(np.diff(ip) >= 2)[0])
    dup = good.copy()
    dup.adj_indices[ip[r] + 1] = dup.adj_indices[ip[r]]                     # one row with a duplicate column
    refused(_bool_plan(dup), "io.triangle_orient")
    wide = io.CSRMatrix(n, n + 128, good.adj_data, good.adj_indices, good.adj_indptr)
    refused(_bool_plan(wide), "num_rows == num_cols")
    with pytest.raises(capi.GraphLilyError) as e:
        plan.tc_count(None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    assert capi.lib().gl_tc_count(None, ctypes.c_void_p(total.ptr), None) == capi.GL_ERR_INVALID_ARG
    still_works()


def test_cpp_driver_equals_the_python_driver(gpu, tmp_path):
    import scipy.sparse as sp
    build_cpp_driver("tc_driver.cpp")
    raw, m, want, _ = _prepared("rmat_20K")
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / "rmat_20K_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([TC_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TriangleCount::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    tc = _driver(raw)
    got = tc.run()
    assert np.array_equal(got, want)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_triangles.bin"), dtype=np.uint64), got)
    assert "triangles: %d\n" % tc.num_triangles_ in r.stdout
    assert "transitivity: %s\n" % repr(tc.transitivity_) in r.stdout or float(r.stdout.split("transitivity: ")[1].split()[0]) == tc.transitivity_
