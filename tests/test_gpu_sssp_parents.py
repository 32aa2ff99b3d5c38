"""GPU parity of weighted SSSP and the shortest-path predecessor tree (gl_sssp_parents, SpMSpVModule.sssp_parents, SSSP.parents,
graphlily::app::SSSP::parents): every comparison is np.array_equal -- distances against the oracle's O.sssp on the test's own
prepared matrix, parents against the numpy statement of the definition (tests/test_sssp_parents_cpu.py) applied to the ORACLE's
distances, plus app.validate_sssp_tree.  (min,+) is order-independent, the definition is exact: no tolerance, no excluded rows."""
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M
from graphlily_amd.dist import partition_rows_by_nnz
from oracle import oracle as O

from helpers import build_cpp_driver
from test_sssp_parents_cpu import (GRAPHS, INF, ITERS, NONE, SHORT, SSSP_DRIVER, WEIGHTINGS, distances_by_definition,
                                   parents_by_definition, prepared_graph, raw_graph, sources, weighted_graph, weights)

pytestmark = pytest.mark.gpu


def _driver(m, weighted=True):
    sssp = app.SSSP(M.num_hbm_channels, 1024, 512, 256, semiring=M.TropicalSemiring)
    assert sssp.semiring_.zero == M.FLOAT_INF
    sssp.set_target("hw")
    sssp.set_up_runtime("unused.xclbin")
    sssp.load_and_format_matrix(m, True, weighted=weighted)
    sssp.send_matrix_host_to_device()
    return sssp


def _check_tree(om, source, ref, sssp, converged, what):
    parent = sssp.parents()
    want, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, ref, source)
    assert parent.dtype == np.uint32 and np.array_equal(parent, want), what
    assert sssp.orphans_ == orphans, what
    if converged:
        assert orphans == 0, what
        assert app.validate_sssp_tree(om, source, ref, parent) == np.count_nonzero(ref < INF), what
    return parent


@pytest.mark.parametrize("kind", WEIGHTINGS)
@pytest.mark.parametrize("name", GRAPHS)
def test_weighted_sssp_and_parents_after_every_mode(gpu, name, kind):
    om = prepared_graph(name, kind)
    sssp = _driver(weighted_graph(name, kind))
    assert sssp.n_ == om.num_rows
    for source in sources(name):
        ref = O.sssp(om, source, ITERS, M.FLOAT_INF)
        assert np.count_nonzero(ref < INF) > 2000
        runs = [("pull", lambda: sssp.pull(source, ITERS)), ("push", lambda: sssp.push(source, ITERS)),
                ("pull_push", lambda: sssp.pull_push(source, ITERS, 0.05))]
        for mode, run in runs:
            what = "%s, %s weights, source %d, %s" % (name, kind, source, mode)
            got = run()
            assert got.dtype == np.float32 and np.array_equal(got, ref), what
            parent = _check_tree(om, source, ref, sssp, True, what)
            # an explicit distance array instead of the last run's
            assert np.array_equal(sssp.parents(ref, source), parent), what
        # cut short: the distances still equal the oracle's, the tree has orphans, and they are counted
        ref5 = O.sssp(om, source, SHORT, M.FLOAT_INF)
        what = "%s, %s weights, source %d, %d iterations" % (name, kind, source, SHORT)
        assert np.array_equal(sssp.pull(source, SHORT), ref5), what
        _check_tree(om, source, ref5, sssp, False, what)
        assert sssp.orphans_ > 0, what
        # ... and an array that is NOT the last run's
        want, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, ref, source)
        assert np.array_equal(sssp.parents(ref, source), want) and sssp.orphans_ == orphans == 0


def test_parents_misuse_is_refused(gpu):
    sssp = _driver(weighted_graph(GRAPHS[0], "int"))
    with pytest.raises(RuntimeError, match="no pull / push / pull_push"):
        sssp.parents()
    d = sssp.pull(0, 3)
    with pytest.raises(ValueError, match="source"):
        sssp.parents(d)
    with pytest.raises(ValueError, match="shape"):
        sssp.parents(d[:-1], 0)
    with pytest.raises(ValueError, match="source"):
        sssp.parents(d, sssp.n_)
    mod = M.SpMSpVModule(512)
    with pytest.raises(SystemExit):
        mod.sssp_parents(None, M.FLOAT_INF, 0, None)
    assert sssp.parents().shape == (sssp.n_,)


@pytest.mark.parametrize("name", GRAPHS[:2])
def test_default_mode_is_untouched(gpu, name):
    """weighted=False: the reference's preparation (every weight 1, some rows without a self edge), distances as before; the
    tree of such distances may have orphans -- a vertex whose row lacks the self edge forgets its distance"""
    raw = weighted_graph(name, "float")
    om = O.CSR(raw.num_rows, raw.num_cols, raw.adj_data, raw.adj_indices, raw.adj_indptr)
    O.sssp_preprocess(om)
    O.util_round_csr_matrix_dim(om, 128, 128)
    assert np.all((om.adj_data == 1) | (om.adj_data == 0))
    sssp = _driver(raw, weighted=False)
    sssp_default = app.SSSP(M.num_hbm_channels, 1024, 512, 256, semiring=M.TropicalSemiring)
    sssp_default.set_up_runtime("unused.xclbin")
    sssp_default.load_and_format_matrix(raw, True)               # the argument left out
    for a, b in ((sssp.SpMV_.csr_matrix_, sssp_default.SpMV_.csr_matrix_), (sssp.SpMSpV_.csc_matrix_, sssp_default.SpMSpV_.csc_matrix_)):
        assert a.adj_indptr.tobytes() == b.adj_indptr.tobytes() and a.adj_indices.tobytes() == b.adj_indices.tobytes()
        assert a.adj_data.tobytes() == b.adj_data.tobytes()
    for source in sources(name):
        ref = O.sssp(om, source, ITERS, M.FLOAT_INF)
        for run in (lambda: sssp.pull(source, ITERS), lambda: sssp.pull_push(source, ITERS, 0.05)):
            assert np.array_equal(run(), ref)
            want, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, ref, source)
            assert np.array_equal(sssp.parents(), want) and sssp.orphans_ == orphans


# ---- the C ABI on plans of the test's own making
def _csc(m):
    c = io.csr2csc(m)
    return capi.SpMSpVPlan(m.num_rows, m.num_cols, c.adj_indptr, c.adj_indices, c.adj_data)


def _run_plan(plan, d, source, unreached=INF, with_orphans=True):
    dist = capi.DeviceBuffer.from_host(np.ascontiguousarray(d, np.float32))
    rows = plan.row_end - plan.row_begin
    par = capi.DeviceBuffer(4 * max(rows, 1))
    cnt = capi.DeviceBuffer.from_host(np.array([12345], np.uint32)) if with_orphans else None
    plan.sssp_parents(dist, unreached, source, par, cnt)
    capi.sync()
    got = par.read(np.uint32, rows) if rows else np.zeros(0, np.uint32)
    return got, (int(cnt.read(np.uint32, 1)[0]) if with_orphans else None)


def _from_coo(n, rows, cols, vals):
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return io.CSRMatrix(n, n, np.asarray(vals, np.float32)[order], np.asarray(cols)[order], indptr)


def _two_long_columns():
    """9216 vertices, four random entries a row, column 5 with more than 9000 entries and column 77 with more than 300 (both
    past the cut: finished by the whole wavefront in full steps of 256 and a partial one; every other column stays below it),
    duplicates of entries with other weights, and weight-0 entries off the diagonal"""
    n = 9216
    rng = np.random.default_rng(31)
    rows = [np.repeat(np.arange(n), 4), rng.choice(n, 9000, replace=False), rng.choice(n, 300, replace=False)]
    cols = [rng.integers(0, n, 4 * n), np.full(9000, 5), np.full(300, 77)]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    dup = rng.choice(rows.shape[0], 3000, replace=False)                  # stored twice, the second time with another weight
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    vals = weights("int", rows.shape[0], 32)
    vals[rng.choice(rows.shape[0], 2000, replace=False)] = 0              # weight-0 entries: edges, but never tree edges
    m = _from_coo(n, rows, cols, vals)
    io.sssp_zero_diagonal(m)
    return m


def test_c_abi_long_columns_duplicates_zero_weights_and_orphans(gpu):
    m = _two_long_columns()
    n = m.num_rows
    col_len = np.bincount(m.adj_indices, minlength=n)
    assert col_len[5] >= 9000 and 300 <= col_len[77] < 400 and np.count_nonzero(col_len > 32) >= 2
    plan = _csc(m)
    for source in (5, 77, 0):
        d, settled = distances_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, source, 40)
        assert settled <= 40 and np.count_nonzero(d < INF) > n // 2
        want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, source)
        got, cnt = _run_plan(plan, d, source)
        assert np.array_equal(got, want) and cnt == orphans
        assert np.count_nonzero(want == 5) > 100, "the long column must father many vertices for the case to mean anything"
        assert np.array_equal(_run_plan(plan, d, source, with_orphans=False)[0], want)        # (d_orphans may be NULL)
    # weight-0 entries off the diagonal tie vertices to equal distances: such a vertex has no strictly nearer predecessor
    assert orphans > 0
    # arrays that are no SSSP result: orphans are counted, not an error
    rng = np.random.default_rng(4)
    for trial in range(3):
        d = rng.integers(0, 12, size=n).astype(np.float32)
        d[rng.random(n) < 0.2] = INF
        source = int(rng.integers(0, n))
        want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, source)
        assert orphans > 0
        got, cnt = _run_plan(plan, d, source)
        assert np.array_equal(got, want) and cnt == orphans
    # another `unreached`
    d = rng.integers(0, 12, size=n).astype(np.float32)
    want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, 3, np.float32(7))
    got, cnt = _run_plan(plan, d, 3, unreached=7.0)
    assert np.array_equal(got, want) and cnt == orphans and np.count_nonzero(want == NONE) > n // 4
    # the measurement hook
    dist = capi.DeviceBuffer.from_host(d)
    par = capi.DeviceBuffer(4 * n)
    read = plan.sssp_parents_entries(dist, 7.0, 3, par)
    assert read == int(col_len[d < 7].sum()) <= m.nnz
    assert np.array_equal(par.read(np.uint32, n), want)


def test_c_abi_unpadded_matrix_and_error_codes(gpu):
    m = weighted_graph("uniform_3000", "float").copy()
    io.sssp_zero_diagonal(m)
    assert m.num_rows == m.num_cols == 3000                      # no multiple of 64
    plan = _csc(m)
    d, _ = distances_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, 7, ITERS)
    want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, 7)
    got, cnt = _run_plan(plan, d, 7)
    assert np.array_equal(got, want) and cnt == orphans == 0
    dist, par = capi.DeviceBuffer.from_host(d), capi.DeviceBuffer(4 * 3000)
    for args, code in (((None, INF, 0, par), capi.GL_ERR_INVALID_ARG), ((dist, INF, 0, None), capi.GL_ERR_INVALID_ARG),
                       ((dist, INF, 3000, par), capi.GL_ERR_INVALID_ARG), ((dist, INF, 0xFFFFFFFF, par), capi.GL_ERR_INVALID_ARG)):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.sssp_parents(*args)
        assert e.value.code == code
    assert capi.lib().gl_sssp_parents(None, capi._p(dist), 1e9, 0, capi._p(par), None) == capi.GL_ERR_INVALID_ARG
    # more rows than columns: the distance vector cannot be indexed by row
    tall = io.CSRMatrix(200, 100, np.ones(200, np.float32), np.arange(200) % 100, np.arange(201))
    tall_plan = _csc(tall)
    with pytest.raises(capi.GraphLilyError) as e:
        tall_plan.sssp_parents(dist, INF, 0, par)
    assert e.value.code == capi.GL_ERR_UNSUPPORTED and "num_rows <= num_cols" in str(e.value)
    # ... and the library goes on working
    assert np.array_equal(_run_plan(plan, d, 7)[0], want)
    assert plan.sssp_parents_entries(dist, INF, 7, par) == m.nnz          # every vertex is reached: every entry is read


@pytest.mark.parametrize("world", [2, 4, 8])
def test_row_shards_on_one_gpu(gpu, world):
    om = prepared_graph("rmat_sym_6016", "int")
    n = om.num_rows
    assert n == 6016
    source = sources("rmat_sym_6016")[1]
    ref = O.sssp(om, source, ITERS, M.FLOAT_INF)
    ref5 = O.sssp(om, source, SHORT, M.FLOAT_INF)
    csc = O.csr2csc(om)
    whole = capi.SpMSpVPlan(n, n, csc.adj_indptr, csc.adj_indices, csc.adj_data)
    bounds = [int(b) for b in partition_rows_by_nnz(om.adj_indptr, world)]
    assert bounds[0] == 0 and bounds[-1] == n
    shards = [capi.SpMSpVPlan(n, n, csc.adj_indptr, csc.adj_indices, csc.adj_data, bounds[k], bounds[k + 1]) for k in range(world)]
    empty = capi.SpMSpVPlan(n, n, csc.adj_indptr, csc.adj_indices, csc.adj_data, bounds[1], bounds[1])
    for d in (ref, ref5):
        want, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d, source)
        got, cnt = _run_plan(whole, d, source)
        assert np.array_equal(got, want) and cnt == orphans
        slices, counts = zip(*[_run_plan(s, d, source) for s in shards])
        assert [s.shape[0] for s in slices] == [bounds[k + 1] - bounds[k] for k in range(world)]
        assert np.array_equal(np.concatenate(slices), want) and sum(counts) == orphans
        for k in range(world):
            assert counts[k] == parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d, source, INF, bounds[k], bounds[k + 1])[1]
        got, cnt = _run_plan(empty, d, source)                   # an empty shard: GL_OK, nothing written, no orphans
        assert got.shape == (0,) and cnt == 0
    assert orphans > 0, "the unfinished run must have orphans for the case to mean anything"


def test_cpp_driver_equals_the_python_driver(gpu, tmp_path):
    import scipy.sparse as sp
    build_cpp_driver("sssp_parents_driver.cpp")
    name, kind = "rmat_sym_4000", "int"
    m = weighted_graph(name, kind)
    A = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int32), m.adj_indptr.astype(np.int32)), shape=(m.num_rows, m.num_cols),
                      dtype=np.float32)
    assert A.nnz == m.nnz
    path = str(tmp_path / "rmat_sym_weighted_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    source = sources(name)[1]
    r = subprocess.run([SSSP_DRIVER, path, str(tmp_path), str(source), str(ITERS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SSSP::parents OK (0 orphans)" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    sssp = _driver(m)
    d = sssp.pull_push(source, ITERS, 0.05)
    p = sssp.parents()
    om = prepared_graph(name, kind)
    assert np.array_equal(d, O.sssp(om, source, ITERS, M.FLOAT_INF))
    assert app.validate_sssp_tree(om, source, d, p) == np.count_nonzero(d < INF)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_distance.bin"), dtype=np.float32), d)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_parents.bin"), dtype=np.uint32), p)
