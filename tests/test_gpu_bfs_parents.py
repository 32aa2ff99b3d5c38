"""GPU parity of the BFS predecessor tree (gl_bfs_parents, SpMVModule.bfs_parents, BFS.parents, graphlily::app::BFS::parents):
every comparison is np.array_equal against the numpy statement of the definition (tests/test_bfs_parents_cpu.py) applied to the
ORACLE's levels, plus app.validate_bfs_tree.  The definition is exact: no tolerance, no excluded rows."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M
from graphlily_amd.dist import partition_rows_by_nnz
from oracle import oracle as O

from helpers import build_cpp_driver, named_matrix, to_oracle
from test_bfs_parents_cpu import NONE, PARENTS_DRIVER, levels_by_definition, parents_by_definition

pytestmark = pytest.mark.gpu

GENERATED = ["uniform_10K_10", "rmat_20K", "rmat_sym_50K", "gplus_small"]
FIXTURES = ["line_8", "eye_10"]
ITERS = 10


def _matrix(name, golden_dir):
    if name in FIXTURES:
        return io.load_csr_matrix_from_float_npz(os.path.join(golden_dir, name + "_csr_float32.npz"))
    return named_matrix(name)


def _oracle_prepared(m):
    om = to_oracle(m)
    O.util_round_csr_matrix_dim(om, 128, 128)
    om.adj_data = np.ones(om.nnz, np.float32)
    return om


def _driver(m):
    bfs = app.BFS(M.num_hbm_channels, 1024, 512, 256)
    bfs.set_target("hw")
    bfs.set_up_runtime("unused.xclbin")
    bfs.load_and_format_matrix(m, True)
    bfs.send_matrix_host_to_device()
    return bfs


def _sources(om):
    """0 and two more, drawn with a fixed seed among the vertices with a non-empty row"""
    lens = np.diff(om.adj_indptr.astype(np.int64))
    pool = np.flatnonzero(lens > 0)
    pool = pool[pool != 0]
    extra = np.random.default_rng(2024).choice(pool, size=min(2, pool.size), replace=False)
    return [0] + [int(s) for s in extra]


def _check(om, source, levels, parent, iters, what):
    want, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, levels)
    assert orphans == 0, what
    assert parent.dtype == np.uint32 and np.array_equal(parent, want), what
    assert app.validate_bfs_tree(om, source, levels, parent, num_iterations=iters) == np.count_nonzero(levels), what


@pytest.mark.parametrize("name", GENERATED + FIXTURES)
def test_parents_after_every_mode(gpu, golden_dir, name):
    m = _matrix(name, golden_dir)
    om = _oracle_prepared(m)
    bfs = _driver(m)
    deepest = 0
    for source in _sources(om):
        ref = O.bfs(om, source, ITERS)
        deepest = max(deepest, ref.max())
        if source == 0 and name in GENERATED:
            assert ref.max() > 2, "source 0 must reach past level 2 for the case to mean anything"
        runs = [("pull", lambda: bfs.pull(source, ITERS)), ("push", lambda: bfs.push(source, ITERS))]
        runs += [("pull_push %g" % thr, lambda thr=thr: bfs.pull_push(source, ITERS, thr)) for thr in (0.1, 0.001, 1.0)]
        for mode, run in runs:
            what = "%s, source %d, %s" % (name, source, mode)
            got = run()
            assert np.array_equal(got, ref), what
            _check(om, source, ref, bfs.parents(), ITERS, what)
            assert bfs.orphans_ == 0
        # an explicit level array instead of the last run's
        assert np.array_equal(bfs.parents(ref), bfs.parents()), "%s, source %d: parents(distance)" % (name, source)
        other = O.bfs(om, source, 2)             # ... also one that is NOT the last run's
        _check(om, source, other, bfs.parents(other), 2, "%s, source %d: parents(levels of 2 iterations)" % (name, source))
    if name in GENERATED:
        assert deepest > 2


def test_iteration_cap_on_the_fixtures(gpu, golden_dir):
    line = _matrix("line_8", golden_dir)         # row v holds column v - 1: a chain from vertex 0
    bfs = _driver(line)
    for run in (lambda: bfs.pull(0, 3), lambda: bfs.push(0, 3), lambda: bfs.pull_push(0, 3, 0.1)):
        d = run()
        assert d[:8].tolist() == [1, 2, 3, 4, 0, 0, 0, 0]
        p = bfs.parents()
        assert p[:4].tolist() == [0, 0, 1, 2] and np.all(p[4:] == NONE)
        assert app.validate_bfs_tree(line, 0, d, p, num_iterations=3) == 4
    eye = _matrix("eye_10", golden_dir)
    bfs = _driver(eye)
    for run in (lambda: bfs.pull(0, 4), lambda: bfs.push(0, 4), lambda: bfs.pull_push(0, 4, 0.1)):
        d = run()
        p = bfs.parents()
        assert p[0] == 0 and np.all(p[1:] == NONE) and np.count_nonzero(d) == 1


def test_shuffled_rows_take_the_full_scan_path(gpu):
    m = named_matrix("rmat_20K")
    om = _oracle_prepared(m)
    bfs = _driver(m)
    sh = m.copy()
    rng = np.random.default_rng(77)
    ip = sh.adj_indptr.astype(np.int64)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(ip[:-1], ip[1:])])
    sh.adj_indices, sh.adj_data = sh.adj_indices[perm], sh.adj_data[perm]
    assert not np.array_equal(sh.adj_indices, m.adj_indices)
    bfs_sh = _driver(sh)
    for source in _sources(om):
        ref = O.bfs(om, source, ITERS)
        assert np.array_equal(bfs.pull_push(source, ITERS, 0.05), ref)
        assert np.array_equal(bfs_sh.pull_push(source, ITERS, 0.05), ref)
        p, p_sh = bfs.parents(), bfs_sh.parents()
        _check(om, source, ref, p, ITERS, "sorted rows, source %d" % source)
        assert np.array_equal(p_sh, p), "shuffled rows, source %d" % source
    assert bfs.SpMV_.plan_.rows_sorted() is True
    assert bfs_sh.SpMV_.plan_.rows_sorted() is False


def _run_plan(plan, levels, with_orphans=True):
    d = capi.DeviceBuffer.from_host(np.ascontiguousarray(levels, np.float32))
    rows = plan.row_end - plan.row_begin
    par = capi.DeviceBuffer(4 * max(rows, 1))
    cnt = capi.DeviceBuffer.from_host(np.array([12345], np.uint32)) if with_orphans else None
    plan.bfs_parents(d, par, cnt)
    capi.sync()
    return par.read(np.uint32, rows), (int(cnt.read(np.uint32, 1)[0]) if with_orphans else None)


def test_c_abi_zero_entries_orphans_and_unsupported_plans(gpu):
    m = datasets.rmat(6016, 90000, seed=21, symmetric=True)       # (6016 = 47 x 128)
    assert m.num_rows == m.num_cols == 6016
    rng = np.random.default_rng(4)
    m.adj_data = np.where(rng.random(m.nnz) < 0.3, 0.0, 1.0).astype(np.float32)
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    ones = np.ones(m.nnz, np.float32)
    differs = False
    for source in (0, 17, 4000):
        d = levels_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, source, 12)
        want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d)
        assert orphans == 0
        got, cnt = _run_plan(plan, d)
        assert np.array_equal(got, want) and cnt == 0
        assert np.array_equal(_run_plan(plan, d, with_orphans=False)[0], want)        # (d_orphans may be NULL)
        # a zero-valued entry is never a parent, although counting it would change the answer somewhere
        differs |= not np.array_equal(parents_by_definition(m.adj_indptr, m.adj_indices, ones, d)[0], want)
    assert differs, "the zero-valued entries must matter for the case to mean anything"
    # level arrays that are no BFS result: orphans are counted, not an error
    for trial in range(3):
        d = rng.integers(0, 5, size=m.num_cols).astype(np.float32)
        want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d)
        assert orphans > 0
        got, cnt = _run_plan(plan, d)
        assert np.array_equal(got, want) and cnt == orphans
    # levels a byte cannot hold (>= 255, fractions): the same call gathers the floats
    d = levels_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, 0, 12)
    for alt in (np.where(d > 0, d + 300, 0), np.where(d > 1, d + 0.5, d)):
        alt = alt.astype(np.float32)
        want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, alt)
        got, cnt = _run_plan(plan, alt)
        assert np.array_equal(got, want) and cnt == orphans
    # a plan without the row copy: GL_ERR_UNSUPPORTED with a message, and the library goes on working
    general = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data)
    assert general.info()["layout"] != "boolean"
    with pytest.raises(capi.GraphLilyError) as e:
        _run_plan(general, d)
    assert e.value.code == capi.GL_ERR_UNSUPPORTED and "row copy" in str(e.value)
    with pytest.raises(capi.GraphLilyError) as e:
        general.rows_sorted()
    assert e.value.code == capi.GL_ERR_UNSUPPORTED
    buf = capi.DeviceBuffer(16)
    with pytest.raises(capi.GraphLilyError) as e:
        plan.bfs_parents(None, buf, None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    want, _ = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d)
    assert np.array_equal(_run_plan(plan, d)[0], want)
    assert plan.bfs_parents_entries(capi.DeviceBuffer.from_host(d), capi.DeviceBuffer(4 * m.num_rows)) <= m.nnz


@pytest.mark.parametrize("world", [2, 4, 8])
def test_row_shards_on_one_gpu(gpu, world):
    om = _oracle_prepared(named_matrix("rmat_sym_50K"))
    n = om.num_rows
    ref = O.bfs(om, 0, ITERS)
    want, _ = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, ref)
    whole = capi.SpMVPlan(n, n, om.adj_indptr, om.adj_indices, om.adj_data, flags=capi.GL_PLAN_BOOLEAN)
    assert np.array_equal(_run_plan(whole, ref)[0], want)
    bounds = partition_rows_by_nnz(om.adj_indptr, world)
    assert all(b % 64 == 0 for b in bounds[:-1]) and bounds[-1] == n
    slices = []
    for k in range(world):
        shard = capi.SpMVPlan(n, n, om.adj_indptr, om.adj_indices, om.adj_data, bounds[k], bounds[k + 1], flags=capi.GL_PLAN_BOOLEAN)
        got, cnt = _run_plan(shard, ref)
        assert cnt == 0 and got.shape[0] == bounds[k + 1] - bounds[k]
        slices.append(got)
    assert np.array_equal(np.concatenate(slices), want)


@pytest.fixture(scope="module")
def orkut(gpu):
    import torch
    m = datasets.paper_graph("orkut", 1.0, device=torch.device("cuda:0"))
    io.util_round_csr_matrix_dim(m, 128, 128)
    return m


def test_full_size_tree_on_the_orkut_stand_in(orkut, gpu):
    raw = orkut
    deg = np.diff(raw.adj_indptr.astype(np.int64))
    src = 0 if deg[0] > 0 else int(np.argmax(deg > 0))
    bfs = _driver(raw)
    d = bfs.pull_push(src, 6, 0.001)
    p = bfs.parents()
    assert bfs.orphans_ == 0 and (d > 0).sum() > raw.num_rows // 2
    ones = np.ones(raw.nnz, np.float32)
    want, orphans = parents_by_definition(raw.adj_indptr, raw.adj_indices, ones, d)
    assert orphans == 0 and np.array_equal(p, want)
    unit = io.CSRMatrix(raw.num_rows, raw.num_cols, ones, raw.adj_indices, raw.adj_indptr)
    assert app.validate_bfs_tree(unit, src, d, p, num_iterations=6) == np.count_nonzero(d)
    assert np.array_equal(bfs.parents(d), p)


def test_cpp_driver_equals_the_python_driver(gpu, tmp_path):
    import scipy.sparse as sp
    build_cpp_driver("bfs_parents_driver.cpp")
    m = named_matrix("rmat_sym_50K")
    A = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int32), m.adj_indptr.astype(np.int32)), shape=(m.num_rows, m.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / "rmat_sym_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([PARENTS_DRIVER, path, str(tmp_path), "0", str(ITERS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BFS::parents OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    bfs = _driver(m)
    d = bfs.pull_push(0, ITERS, 0.05)
    p = bfs.parents()
    om = _oracle_prepared(m)
    _check(om, 0, O.bfs(om, 0, ITERS), p, ITERS, "python driver")
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_levels.bin"), dtype=np.float32), d)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_parents.bin"), dtype=np.uint32), p)
