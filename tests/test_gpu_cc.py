"""GPU parity of the weakly connected components (gl_cc_begin / gl_cc_hook / gl_cc_finish / gl_cc_labels, SpMVModule.cc_labels,
app.ConnectedComponents, graphlily::app::ConnectedComponents): every comparison is np.array_equal against the numpy statement of
the definition (tests/test_cc_cpu.py) on the prepared matrix.  The definition is exact: no tolerance, no excluded vertices."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M
from graphlily_amd.dist import partition_rows_by_nnz

from helpers import build_cpp_driver, named_matrix
from test_cc_cpu import CC_DRIVER, ROOT, components_by_definition, many_components, permute_rows

pytestmark = pytest.mark.gpu

GENERATED = ["uniform_10K_10", "rmat_20K", "rmat_sym_50K", "gplus_small"]
FIXTURES = ["line_8", "eye_10"]
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """-> (the matrix as given, the matrix as the drivers prepare it: padded to 128, every entry 1, its labels, its count);
    computed once and shared, never written"""
    if name in FIXTURES:
        raw = io.load_csr_matrix_from_float_npz(os.path.join(GOLDEN, name + "_csr_float32.npz"))
    elif name == "many":
        raw = many_components()
    else:
        raw = named_matrix(name)
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    m.adj_data = np.ones(m.nnz, np.float32)
    labels, count = components_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, m.num_rows)
    labels.setflags(write=False)
    return raw, m, labels, count


def _driver(m):
    cc = app.ConnectedComponents(M.num_hbm_channels, 1024, 256)
    cc.set_target("hw")
    cc.set_up_runtime("unused.xclbin")
    cc.load_and_format_matrix(m, True)
    cc.send_matrix_host_to_device()
    return cc


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean"
    return plan


def _labels_of(plan, n, with_count=True):
    lab = capi.DeviceBuffer(4 * n)
    cnt = capi.DeviceBuffer.from_host(np.array([12345], np.uint32)) if with_count else None
    plan.cc_labels(lab, cnt)
    capi.sync()
    return lab.read(np.uint32, n), (int(cnt.read(np.uint32, 1)[0]) if with_count else None)


def _csr(n, rows, cols, data=None):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    data = np.ones(rows.shape[0], np.float32) if data is None else np.asarray(data, np.float32)[order]
    return io.CSRMatrix(n, n, data, cols.astype(np.uint32), np.cumsum(indptr).astype(np.uint32))


@pytest.mark.parametrize("name", GENERATED + FIXTURES + ["many"])
def test_drivers(gpu, name):
    raw, m, want, count = _prepared(name)
    cc = _driver(raw)
    got = cc.run()
    assert got.dtype == np.uint32 and got.shape == (m.num_rows,) and np.array_equal(got, want)
    assert cc.n_real_ == raw.num_rows and cc.num_components_ == count - (m.num_rows - raw.num_rows)
    assert cc.largest_component_ == np.bincount(want).max()
    assert app.validate_components(m, got) == count
    assert np.array_equal(cc.run(), got)
    if name == "many":
        import scipy.sparse as sp
        S = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int64), m.adj_indptr.astype(np.int64)), shape=(m.num_rows, m.num_cols))
        assert (S != S.T).nnz > 0, "entries are stored one way only"
        assert np.count_nonzero(np.bincount(want) > 1) == 900


@pytest.mark.parametrize("numbering", ["ascending", "descending", "shuffled"])
def test_a_path_of_a_million_vertices(gpu, numbering):
    """the chain-length case: hooked in index order the forest is one chain, which neither the find nor the finish may walk
    vertex by vertex"""
    n = 1 << 20
    v = np.arange(1, n, dtype=np.int64)
    if numbering == "ascending":
        m = _csr(n, v, v - 1)                    # A[v, v - 1]
    elif numbering == "descending":
        m = _csr(n, v - 1, v)                    # A[v, v + 1]
    else:
        name = np.random.default_rng(9).permutation(n)
        m = _csr(n, name[v], name[v - 1])
    got, cnt = _labels_of(_bool_plan(m), n)
    assert cnt == 1 and not got.any()            # the path holds every vertex: its smallest is 0


@pytest.mark.parametrize("centre", ["first", "last"])
@pytest.mark.parametrize("shape", ["one long row", "a hundred thousand short rows"])
def test_stars(gpu, shape, centre):
    """a row far past the cut (the wavefront takes it over), and its transpose: every row hooks onto one root"""
    leaves, n = 100000, 100096
    c = 0 if centre == "first" else leaves
    others = np.arange(leaves + 1)
    others = others[others != c]
    m = _csr(n, np.full(leaves, c), others) if shape == "one long row" else _csr(n, others, np.full(leaves, c))
    want = np.arange(n, dtype=np.uint32)
    want[:leaves + 1] = 0
    assert np.array_equal(components_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, n)[0], want)
    got, cnt = _labels_of(_bool_plan(m), n)
    assert np.array_equal(got, want) and cnt == n - leaves


def test_c_abi_details(gpu):
    m = datasets.rmat(6016, 12000, seed=21, symmetric=False)       # (6016 = 47 x 128; sparse enough for many components)
    assert m.num_rows == m.num_cols == 6016
    n = m.num_rows
    rng = np.random.default_rng(4)
    m.adj_data = np.where(rng.random(m.nnz) < 0.3, 0.0, 1.0).astype(np.float32)
    want, count = components_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, n)
    every, every_count = components_by_definition(m.adj_indptr, m.adj_indices, None, n)
    assert every_count < count and 1 < count < n, "the zero-valued entries must matter for the case to mean anything"
    plan = _bool_plan(m)
    got, cnt = _labels_of(plan, n)
    assert np.array_equal(got, want) and cnt == count
    assert app.validate_components(m, got) == count
    assert np.array_equal(_labels_of(plan, n, with_count=False)[0], want)            # (d_count may be NULL)
    # unsorted rows give the same labels
    sh = permute_rows(m, 77)
    assert not np.array_equal(sh.adj_indices, m.adj_indices)
    got_sh, cnt_sh = _labels_of(_bool_plan(sh), n)
    assert np.array_equal(got_sh, want) and cnt_sh == count
    # the three steps by hand, and what they refuse
    parent, labels = capi.DeviceBuffer(4 * n), capi.DeviceBuffer(4 * n)
    capi.cc_begin(parent, n)
    capi.sync()
    assert np.array_equal(parent.read(np.uint32, n), np.arange(n, dtype=np.uint32))
    plan.cc_hook(parent)
    capi.sync()
    forest = parent.read(np.uint32, n)
    assert np.all(forest <= np.arange(n)) and np.array_equal(want[forest], want)     # the invariant: parent[x] <= x, in x's component
    with pytest.raises(capi.GraphLilyError) as e:
        capi.cc_finish(parent, n, parent)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    for call in (lambda: capi.cc_finish(parent, n, None), lambda: capi.cc_finish(None, n, labels), lambda: capi.cc_begin(None, n),
                 lambda: plan.cc_hook(None), lambda: plan.cc_labels(None)):
        with pytest.raises(capi.GraphLilyError) as e:
            call()
        assert e.value.code == capi.GL_ERR_INVALID_ARG
    capi.cc_finish(parent, n, labels)
    capi.sync()
    assert np.array_equal(labels.read(np.uint32, n), want)
    # a plan without the row copy: GL_ERR_UNSUPPORTED with a message, and the library goes on working
    general = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data)
    assert general.info()["layout"] != "boolean"
    for call in (lambda: general.cc_labels(labels), lambda: general.cc_hook(parent)):
        with pytest.raises(capi.GraphLilyError) as e:
            call()
        assert e.value.code == capi.GL_ERR_UNSUPPORTED and "row copy" in str(e.value)
    assert np.array_equal(_labels_of(plan, n)[0], want)


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("name", ["rmat_sym_50K", "many"])
def test_shards_hooked_into_one_forest(gpu, name, world):
    _, m, want, count = _prepared(name)
    n = m.num_rows
    got, cnt = _labels_of(_bool_plan(m), n)
    assert np.array_equal(got, want) and cnt == count
    bounds = partition_rows_by_nnz(m.adj_indptr, world)
    assert all(b % 64 == 0 for b in bounds[:-1]) and bounds[-1] == n
    shards = [_bool_plan(m, bounds[k], bounds[k + 1]) for k in range(world)]
    for order in (shards, shards[::-1]):
        parent, labels = capi.DeviceBuffer(4 * n), capi.DeviceBuffer(4 * n)
        cnt = capi.DeviceBuffer.from_host(np.array([12345], np.uint32))
        capi.cc_begin(parent, n)
        for plan in order:
            plan.cc_hook(parent)
        capi.cc_finish(parent, n, labels, cnt)
        capi.sync()
        assert np.array_equal(labels.read(np.uint32, n), got) and int(cnt.read(np.uint32, 1)[0]) == count
    # one shard alone: the components of its own entries
    ip = m.adj_indptr.astype(np.int64)
    for k in (0, world - 1):
        only = np.zeros(m.nnz, np.float32)
        only[ip[bounds[k]]:ip[bounds[k + 1]]] = 1
        alone, alone_count = components_by_definition(m.adj_indptr, m.adj_indices, only, n)
        assert alone_count > count
        got_k, cnt_k = _labels_of(shards[k], n)
        assert np.array_equal(got_k, alone) and cnt_k == alone_count


def test_cpp_driver_equals_the_python_driver(gpu, tmp_path):
    import scipy.sparse as sp
    build_cpp_driver("cc_driver.cpp")
    raw, m, want, count = _prepared("rmat_20K")
    A = sp.csr_matrix((raw.adj_data, raw.adj_indices.astype(np.int32), raw.adj_indptr.astype(np.int32)), shape=(raw.num_rows, raw.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / "rmat_20K_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([CC_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ConnectedComponents::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    cc = _driver(raw)
    got = cc.run()
    assert np.array_equal(got, want)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_labels.bin"), dtype=np.uint32), got)
    assert "components: %d\n" % cc.num_components_ in r.stdout and "largest: %d\n" % cc.largest_component_ in r.stdout
