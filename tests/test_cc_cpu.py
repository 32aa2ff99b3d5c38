"""CPU suite of the weakly connected components (gl_cc_begin / gl_cc_hook / gl_cc_finish / gl_cc_labels, SpMVModule.cc_labels,
app.ConnectedComponents, app.validate_components): the exports and their bindings exist, the numpy statement of the definition
(kept here; tests/test_gpu_cc.py compares the kernels with it bit for bit) agrees with scipy on generated graphs, with and
without zero-valued entries and whatever the order of a row's entries, the host-side validator accepts a correct labelling and
rejects each kind of wrong one, the driver refuses what it cannot do, and the C++ driver compiles against include/ and fails
loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver, named_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_DRIVER = os.path.join(ROOT, "build", "cc_driver")
SYMBOLS = ("gl_cc_begin", "gl_cc_hook", "gl_cc_finish", "gl_cc_labels")


def components_by_definition(indptr, indices, data, n):
    """The definition, in numpy: -> (labels as uint32[n], count).  An entry (v, u) of row v is an edge unless its value is 0 or
    u >= n (data None: every stored entry counts); labels[v] = the smallest vertex joined to v by a chain of edges taken in
    either direction; count = number of v with labels[v] == v.  A union-find whose unions are done a round at a time: parent[x]
    <= x throughout, every round hooks the larger root of each edge under the smallest root some edge offers it, then every
    vertex is pointed at its root."""
    indptr = np.asarray(indptr).astype(np.int64)
    nr = indptr.shape[0] - 1
    rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(indptr))
    cols = np.asarray(indices[:indptr[nr]]).astype(np.int64)
    keep = (cols < n) & (rows < n) & (cols != rows)
    if data is not None:
        keep &= np.asarray(data[:indptr[nr]]) != 0
    a, b = rows[keep], cols[keep]
    parent = np.arange(n, dtype=np.int64)
    while a.size:
        ra, rb = parent[a], parent[b]                    # (roots: the array is fully compressed between rounds)
        differ = ra != rb
        a, b, ra, rb = a[differ], b[differ], ra[differ], rb[differ]      # an edge inside one tree never matters again
        if not a.size:
            break
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        order = np.lexsort((lo, hi))                     # per larger root, the smallest offer first
        hi, lo = hi[order], lo[order]
        lead = np.concatenate(([True], hi[1:] != hi[:-1]))
        parent[hi[lead]] = lo[lead]
        while True:
            jump = parent[parent]
            if np.array_equal(jump, parent):
                break
            parent = jump
    labels = parent.astype(np.uint32)
    return labels, int(np.count_nonzero(parent == np.arange(n)))


def scipy_min_labels(indptr, indices, data, n):
    """scipy's weak components of the same edge set, every class renamed to its smallest vertex -> (labels, count)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    indptr = np.asarray(indptr).astype(np.int64)
    nr = indptr.shape[0] - 1
    rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(indptr))
    cols = np.asarray(indices[:indptr[nr]]).astype(np.int64)
    keep = (cols < n) & (rows < n)
    if data is not None:
        keep &= np.asarray(data[:indptr[nr]]) != 0
    A = sp.csr_matrix((np.ones(int(keep.sum()), np.int8), (rows[keep], cols[keep])), shape=(n, n))
    count, comp = connected_components(A, directed=True, connection="weak")
    smallest = np.full(count, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.uint32), int(count)


def permute_rows(m, seed):
    """a copy of the matrix with the entries of every row in a random order"""
    rng = np.random.default_rng(seed)
    ip = m.adj_indptr.astype(np.int64)
    row_of = np.repeat(np.arange(m.num_rows), np.diff(ip))
    perm = np.lexsort((rng.random(row_of.shape[0]), row_of))
    out = m.copy()
    out.adj_indices, out.adj_data = m.adj_indices[perm], m.adj_data[perm]
    return out


def many_components(seed=31):
    """A disjoint union of 300 paths, 300 cycles and 300 stars with 2..200 vertices each, vertex numbers shuffled, every edge stored
    ONE way only in a random direction, padded to a multiple of 128 (the padding vertices are singletons) -> CSRMatrix"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 201, size=900)
    src, dst, base = [], [], 0
    for k, s in enumerate(sizes):
        v = np.arange(base, base + s)
        if k < 300:                                  # path
            a, b = v[:-1], v[1:]
        elif k < 600:                                # cycle (of two vertices: one doubled edge)
            a, b = v, np.roll(v, -1)
        else:                                        # star
            a, b = np.full(s - 1, v[0]), v[1:]
        src.append(a)
        dst.append(b)
        base += s
    src, dst = np.concatenate(src), np.concatenate(dst)
    n = (base + 127) // 128 * 128
    rename = rng.permutation(n)
    src, dst = rename[src], rename[dst]
    flip = rng.random(src.shape[0]) < 0.5
    rows, cols = np.where(flip, dst, src), np.where(flip, src, dst)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr)
    return io.CSRMatrix(n, n, np.ones(rows.shape[0], np.float32), cols.astype(np.uint32), indptr.astype(np.uint32))


def test_library_exports_and_binds_the_four_entry_points():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "graphlily_hip.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), "libgraphlily_hip.so does not export %s" % sym
        assert sym in capi.EXPORTS
    assert [len(getattr(L, s).argtypes) for s in SYMBOLS] == [2, 2, 4, 3]
    for decl in ("int gl_cc_begin(uint32_t *d_parent, uint32_t n);",
                 "int gl_cc_hook(gl_spmv_plan plan, uint32_t *d_parent);",
                 "int gl_cc_finish(uint32_t *d_parent, uint32_t n, uint32_t *d_labels, uint32_t *d_count /* may be NULL */);",
                 "int gl_cc_labels(gl_spmv_plan plan, uint32_t *d_labels, uint32_t *d_count /* may be NULL */);"):
        assert decl in header
    assert callable(capi.SpMVPlan.cc_labels) and callable(capi.SpMVPlan.cc_hook) and callable(capi.cc_begin) and callable(capi.cc_finish)
    assert callable(M.SpMVModule.cc_labels) and callable(app.ConnectedComponents.run) and callable(app.validate_components)
    assert "cc_labels(DeviceBuffer labels" in open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()


def test_compute_entry_points_fail_loudly_without_a_gpu():
    if capi.device_count() == 0:
        L = capi.lib()
        assert L.gl_cc_labels(None, None, None) == capi.GL_ERR_NOT_INITIALIZED
        assert L.gl_cc_begin(None, 0) == capi.GL_ERR_NOT_INITIALIZED
        assert L.gl_cc_hook(None, None) == capi.GL_ERR_NOT_INITIALIZED
        assert L.gl_cc_finish(None, 0, None, None) == capi.GL_ERR_NOT_INITIALIZED


GRAPHS = {
    "uniform": lambda: datasets.uniform(3000, 4, seed=5),
    "rmat": lambda: datasets.rmat(4000, 30000, seed=6),
    "rmat_sym": lambda: datasets.rmat(4000, 40000, seed=8, symmetric=True),
    "rmat_20K": lambda: named_matrix("rmat_20K"),
    "gplus_small": lambda: named_matrix("gplus_small"),
    "rmat_sym_50K": lambda: named_matrix("rmat_sym_50K"),
}
# (components, vertices in the largest, non-singleton components), counted on the CPU
FACTS = {"rmat_20K": (4109, 15892, None), "gplus_small": (778, None, None), "rmat_sym_50K": (14087, None, 10)}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_definition_agrees_with_scipy(graph):
    m = GRAPHS[graph]()
    n = max(m.num_rows, m.num_cols)
    labels, count = components_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, n)
    want, want_count = scipy_min_labels(m.adj_indptr, m.adj_indices, m.adj_data, n)
    assert labels.dtype == np.uint32 and np.array_equal(labels, want) and count == want_count
    assert app.validate_components(m, labels) == count
    if graph in FACTS:
        comps, largest, big = FACTS[graph]
        sizes = np.bincount(labels)
        assert count == comps
        assert largest is None or sizes.max() == largest
        assert big is None or np.count_nonzero(sizes > 1) == big
    # a tenth of the entries zeroed: they are no edges
    z = m.copy()
    z.adj_data = np.where(np.random.default_rng(1).random(m.nnz) < 0.1, 0.0, 1.0).astype(np.float32)
    zl, zc = components_by_definition(z.adj_indptr, z.adj_indices, z.adj_data, n)
    want, want_count = scipy_min_labels(z.adj_indptr, z.adj_indices, z.adj_data, n)
    assert np.array_equal(zl, want) and zc == want_count and zc >= count
    assert app.validate_components(z, zl) == zc
    # the order of a row's entries does not matter
    p = permute_rows(z, 3)
    assert not np.array_equal(p.adj_indices, z.adj_indices)
    pl, pc = components_by_definition(p.adj_indptr, p.adj_indices, p.adj_data, n)
    assert np.array_equal(pl, zl) and pc == zc


def test_the_many_component_graph_is_what_it_claims():
    m = many_components()
    assert m.num_rows % 128 == 0
    import scipy.sparse as sp
    A = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int64), m.adj_indptr.astype(np.int64)), shape=(m.num_rows, m.num_cols))
    assert (A != A.T).nnz > 0, "entries are stored one way only"
    labels, count = components_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, m.num_rows)
    assert np.count_nonzero(np.bincount(labels) > 1) == 900
    want, want_count = scipy_min_labels(m.adj_indptr, m.adj_indices, m.adj_data, m.num_rows)
    assert np.array_equal(labels, want) and count == want_count
    assert app.validate_components(m, labels) == count


def _two_triangles_and_a_tail():
    """vertices 0-1-2 and 3-4-5 (triangles, entries one way), 6-7 (an edge), 8 alone; 10 labels (one padding vertex)"""
    rows = np.array([1, 2, 2, 4, 5, 5, 7])
    cols = np.array([0, 0, 1, 3, 3, 4, 6])
    indptr = np.zeros(10, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    m = io.CSRMatrix(9, 9, np.ones(7, np.float32), cols.astype(np.uint32), np.cumsum(indptr).astype(np.uint32))
    return m, np.array([0, 0, 0, 3, 3, 3, 6, 6, 8, 9], dtype=np.uint32)


@pytest.mark.parametrize("what,rule", [("a label that is not the minimum of its class", 1), ("an entry that crosses two classes", 2),
                                       ("one class split in two", 2), ("two classes merged", 3), ("a label that is not idempotent", 1),
                                       ("a class that is not connected", 3)])
def test_validator_rejects(what, rule):
    m, labels = _two_triangles_and_a_tail()
    assert app.validate_components(m, labels) == 5
    assert np.array_equal(components_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, 10)[0], labels)
    bad = labels.copy()
    if what == "a label that is not the minimum of its class":
        bad[3:6] = 4                            # the class {3, 4, 5} named after 4
    elif what == "an entry that crosses two classes":
        bad[2] = 2                              # A[2, 0] and A[2, 1] now leave the class {2}
    elif what == "one class split in two":
        bad[7] = 7                              # {6, 7} cut into {6} and {7}: the entry A[7, 6] crosses
    elif what == "two classes merged":
        bad[3:6] = 0                            # {0, 1, 2} and {3, 4, 5} under one label, and nothing joins them
    elif what == "a label that is not idempotent":
        bad[5] = 4                              # 5 -> 4 -> 3
    else:
        bad[8] = 6                              # vertex 8 has no entry at all, yet sits in the class of 6
    with pytest.raises(ValueError, match=r"\(rule %d\)" % rule):
        app.validate_components(m, bad)
    with pytest.raises(ValueError, match="labels for a"):
        app.validate_components(m, labels[:8])


class _TwoRanks:
    """what the drivers ask of a communicator, claiming rank 0 of 2"""
    rank, world_size, distributed = 0, 2, True


def test_driver_refuses_row_shards_and_a_run_before_send(golden_dir):
    with pytest.raises(NotImplementedError, match="gl_cc_hook"):
        app.ConnectedComponents(comm=_TwoRanks(), backend=CpuBackend())
    cc = app.ConnectedComponents(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        cc.run()
    cc.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (cc.n_, cc.n_real_) == (128, 8)
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        cc.run()


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("cc_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([CC_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
