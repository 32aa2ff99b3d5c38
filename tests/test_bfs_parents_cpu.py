"""CPU suite of the BFS predecessor tree (gl_bfs_parents, BFS.parents, validate_bfs_tree): the export and its binding exist,
the host-side validator accepts a correct tree and rejects each kind of wrong one, the numpy statement of the definition
(kept here; tests/test_gpu_bfs_parents.py compares the kernel with it bit for bit) agrees with the validator on random
graphs, and the C++ driver compiles against include/ and fails loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io

from helpers import build_cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENTS_DRIVER = os.path.join(ROOT, "build", "bfs_parents_driver")
NONE = np.uint32(0xFFFFFFFF)


def parents_by_definition(indptr, indices, data, d, row_begin=0, row_end=None):
    """The definition, in numpy: for the rows [row_begin, row_end) of the CSR (row v lists the vertices v is pulled from) and
    the level array d -> (parent[row_begin:row_end] as uint32, number of orphans).  parent[v] = v where d[v] == 1, 0xffffffff
    where d[v] == 0, otherwise min{u : A[v, u] != 0 and d[u] == d[v] - 1} -- 0xffffffff and one orphan if there is no such u."""
    indptr = np.asarray(indptr).astype(np.int64)
    d = np.asarray(d, dtype=np.float32)
    row_end = indptr.shape[0] - 1 if row_end is None else row_end
    par = np.full(row_end - row_begin, NONE, dtype=np.uint32)
    step = 1 << 18                                  # rows per block (bounds the temporaries at 2e8 entries)
    for r0 in range(row_begin, row_end, step):
        r1 = min(row_end, r0 + step)
        lo, hi = indptr[r0], indptr[r1]
        lens = np.diff(indptr[r0:r1 + 1])
        rows = np.repeat(np.arange(r0, r1), lens)
        cols = np.asarray(indices[lo:hi])
        ok = (np.asarray(data[lo:hi]) != 0) & (d[cols] == d[rows] - np.float32(1))
        cand = np.append(np.where(ok, cols, NONE).astype(np.uint32), NONE)        # (+ a sentinel: reduceat needs valid starts)
        best = np.minimum.reduceat(cand, indptr[r0:r1] - lo)
        par[r0 - row_begin:r1 - row_begin] = np.where(lens > 0, best, NONE)
    dv = d[row_begin:row_end]
    v = np.arange(row_begin, row_end, dtype=np.uint32)
    par = np.where(dv == 0, NONE, np.where(dv == 1, v, par)).astype(np.uint32)
    return par, int(np.count_nonzero((dv != 0) & (dv != 1) & (par == NONE)))


def levels_by_definition(indptr, indices, data, source, num_iterations):
    """The drivers' levels by plain frontier expansion over the rows (numpy): 1 on the source, it + 1 for a vertex reached in
    iteration it, 0 = not reached."""
    indptr = np.asarray(indptr).astype(np.int64)
    n = indptr.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    cols, live = np.asarray(indices).astype(np.int64), np.asarray(data) != 0
    d = np.zeros(max(n, int(cols.max(initial=0)) + 1), dtype=np.float32)
    d[source] = 1
    for it in range(1, num_iterations + 1):
        hit = np.zeros(d.shape[0], dtype=bool)
        hit[rows[live & (d[cols] == it)]] = True
        d[hit & (d == 0)] = it + 1
    return d


def test_library_exports_and_binds_gl_bfs_parents():
    L = capi.lib()
    for sym in ("gl_bfs_parents", "gl_bfs_parents_entries", "gl_spmv_plan_rows_sorted"):
        assert hasattr(L, sym), "libgraphlily_hip.so does not export %s" % sym
        assert sym in capi.EXPORTS
    assert L.gl_bfs_parents.argtypes is not None and len(L.gl_bfs_parents.argtypes) == 4
    assert callable(getattr(capi.SpMVPlan, "bfs_parents")) and callable(getattr(capi.SpMVPlan, "rows_sorted"))
    from graphlily_amd import module as M
    assert callable(getattr(M.SpMVModule, "bfs_parents")) and callable(getattr(app.BFS, "parents"))
    header = open(os.path.join(ROOT, "include", "graphlily_hip.h")).read()
    assert "int gl_bfs_parents(gl_spmv_plan plan, const float *d_distance, uint32_t *d_parent, uint32_t *d_orphans);" in header


def test_compute_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        rc = capi.lib().gl_bfs_parents(None, None, None, None)
        assert rc == capi.GL_ERR_NOT_INITIALIZED


def _line8(golden_dir):
    m = io.load_csr_matrix_from_float_npz(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    d = np.arange(1, 9, dtype=np.float32)                       # row v holds column v - 1: a chain from vertex 0
    p = np.array([0, 0, 1, 2, 3, 4, 5, 6], dtype=np.uint32)
    return m, d, p


def test_validator_accepts_a_hand_made_tree(golden_dir):
    m, d, p = _line8(golden_dir)
    assert app.validate_bfs_tree(m, 0, d, p) == 8
    assert app.validate_bfs_tree(m, 0, d, p, num_iterations=7) == 8
    # three iterations: levels 1..4 on vertices 0..3, nothing behind them -- vertex 3 (the last level) was never expanded
    d3, p3 = d.copy(), p.copy()
    d3[4:], p3[4:] = 0, NONE
    assert app.validate_bfs_tree(m, 0, d3, p3, num_iterations=3) == 4
    with pytest.raises(ValueError, match="rule 5"):
        app.validate_bfs_tree(m, 0, d3, p3)                     # without the cap, 3 -> 4 is an edge nobody followed
    got, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d3)
    assert np.array_equal(got, p3) and orphans == 0


def _line8_with_a_shortcut(golden_dir):
    """line_8 plus the entry A[5, 3]: vertices 4 and 5 share level 5, so a parent can sit on the right level and still be no
    neighbour."""
    m, _, _ = _line8(golden_dir)
    m.adj_indptr = np.array([0, 0, 1, 2, 3, 4, 6, 7, 8], dtype=np.uint32)
    m.adj_indices = np.array([0, 1, 2, 3, 3, 4, 5, 6], dtype=np.uint32)
    m.adj_data = np.ones(8, dtype=np.float32)
    d = np.array([1, 2, 3, 4, 5, 5, 6, 7], dtype=np.float32)
    p = np.array([0, 0, 1, 2, 3, 3, 5, 6], dtype=np.uint32)
    return m, d, p


@pytest.mark.parametrize("what,rule", [("parent is no neighbour", 3), ("parent on the wrong level", 4), ("reached vertex without parent", 2),
                                       ("parent on an unreached vertex", 4), ("unreached vertex with a parent", 2),
                                       ("source is not its own parent", 1), ("an edge skips a level", 5)])
def test_validator_rejects(golden_dir, what, rule):
    m, d, p = _line8_with_a_shortcut(golden_dir)
    assert app.validate_bfs_tree(m, 0, d, p) == 8
    got, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d)
    assert np.array_equal(got, p) and orphans == 0
    cap = None
    if what == "parent is no neighbour":
        p[6] = 4                        # level 5, one above vertex 6 -- but A[6, 4] is no entry
    elif what == "parent on the wrong level":
        p[5] = 4                        # A[5, 4] is an entry, but 4 sits on vertex 5's own level
    elif what == "reached vertex without parent":
        p[6] = NONE
    elif what == "parent on an unreached vertex":
        d[6], p[6] = 0, NONE            # 7 keeps level 7 and parent 6, which is no longer reached
    elif what == "unreached vertex with a parent":
        d[6:], p[6] = 0, NONE           # the search stopped after 4 iterations (levels <= 5); 7 still names a parent
        cap = 4
    elif what == "source is not its own parent":
        p[0] = 1
    else:
        d[5:], p[5] = [6, 7, 8], 4      # a tree through 4 that obeys rules 1-4, but the entry A[5, 3] leads from level 4 to level 6
    with pytest.raises(ValueError, match=r"\(rule %d\)" % rule):
        app.validate_bfs_tree(m, 0, d, p, num_iterations=cap)


@pytest.mark.parametrize("graph", ["uniform", "rmat", "rmat_sym"])
def test_definition_agrees_with_the_validator_on_random_graphs(graph):
    m = {"uniform": lambda: datasets.uniform(3000, 4, seed=5),
         "rmat": lambda: datasets.rmat(4000, 30000, seed=6),
         "rmat_sym": lambda: datasets.rmat(4000, 40000, seed=8, symmetric=True)}[graph]()
    rng = np.random.default_rng(1)
    m.adj_data = np.where(rng.random(m.nnz) < 0.1, 0.0, 1.0).astype(np.float32)     # explicit zeros are no edges
    lens = np.diff(m.adj_indptr.astype(np.int64))
    sources = [int(s) for s in rng.choice(np.flatnonzero(lens[:m.num_cols] > 0), size=3, replace=False)]
    deep = 0
    for source in sources:
        for cap in (2, 40):
            d = levels_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, source, cap)
            par, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d)
            assert orphans == 0 and par[source] == source
            reached = app.validate_bfs_tree(m, source, d[:par.shape[0]], par, num_iterations=cap)
            assert reached == np.count_nonzero(d)
            deep = max(deep, d.max())
            # the result does not depend on the order of a row's entries
            perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(m.adj_indptr[:-1].astype(np.int64), m.adj_indptr[1:].astype(np.int64))]).astype(np.int64) if m.nnz else np.zeros(0, np.int64)
            par2, _ = parents_by_definition(m.adj_indptr, m.adj_indices[perm], m.adj_data[perm], d)
            assert np.array_equal(par, par2)
            # a damaged tree does not pass
            kids = np.flatnonzero(d >= 3)
            if kids.size:
                bad = par.copy()
                bad[kids[0]] = source if d[kids[0]] > 3 or par[kids[0]] != source else kids[0]
                with pytest.raises(ValueError):
                    app.validate_bfs_tree(m, source, d[:par.shape[0]], bad, num_iterations=cap)
    assert deep > 3, "the searches must reach past level 3 for the case to mean anything"


def test_orphans_of_a_level_array_that_is_no_bfs_result(golden_dir):
    m, d, _ = _line8(golden_dir)
    d = np.array([1, 2, 5, 6, 0, 3, 4, 9], dtype=np.float32)
    par, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d)
    assert par.tolist() == [0, 0, NONE, 2, NONE, NONE, 5, NONE] and orphans == 3


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("bfs_parents_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([PARENTS_DRIVER, str(tmp_path / "none.npz"), str(tmp_path), "0", "4"], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
