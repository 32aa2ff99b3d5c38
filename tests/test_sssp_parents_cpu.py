"""CPU suite of weighted SSSP and the shortest-path predecessor tree (gl_sssp_parents, SSSP.parents, io.sssp_zero_diagonal,
validate_sssp_tree): the exports and their bindings exist, the weighted preparation does what it says, the host-side validator
accepts a correct tree and rejects one wrong one per rule, the numpy statement of the definition (kept here;
tests/test_gpu_sssp_parents.py compares the kernel with it bit for bit) agrees with the validator on random weighted graphs,
and the C++ driver compiles against include/ and fails loudly without a GPU.  (min,+) is order-independent -- fl(d[u] + w) is
formed per entry, min is exact -- so every comparison is exact."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, datasets, io, module as M
from oracle import oracle as O

from helpers import build_cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSSP_DRIVER = os.path.join(ROOT, "build", "sssp_parents_driver")
NONE = np.uint32(0xFFFFFFFF)
INF = np.float32(M.FLOAT_INF)
GRAPHS = ["uniform_3000", "rmat_4000", "rmat_sym_4000", "rmat_sym_6016"]
WEIGHTINGS = ["int", "float"]
ITERS, SHORT = 24, 5


def parents_by_definition(indptr, indices, data, d, source, unreached=INF, row_begin=0, row_end=None):
    """The definition, in numpy: for the rows [row_begin, row_end) of the CSR (row v lists the vertices v is pulled from) and the
    distance array d -> (parent[row_begin:row_end] as uint32, number of orphans).  parent[source] = source, 0xffffffff where
    d[v] >= unreached, otherwise min{u : A[v, u] stored with weight w, d[u] < d[v] and fl(d[u] + w) == d[v]} -- 0xffffffff and one
    orphan if there is no such u."""
    indptr = np.asarray(indptr).astype(np.int64)
    d = np.asarray(d, dtype=np.float32)
    unreached = np.float32(unreached)
    row_end = indptr.shape[0] - 1 if row_end is None else row_end
    par = np.full(row_end - row_begin, NONE, dtype=np.uint32)
    step = 1 << 18                                  # rows per block (bounds the temporaries at 2e8 entries)
    for r0 in range(row_begin, row_end, step):
        r1 = min(row_end, r0 + step)
        lo, hi = indptr[r0], indptr[r1]
        lens = np.diff(indptr[r0:r1 + 1])
        rows = np.repeat(np.arange(r0, r1), lens)
        cols = np.asarray(indices[lo:hi]).astype(np.int64)
        w = np.asarray(data[lo:hi], dtype=np.float32)
        ok = (d[cols] < d[rows]) & (d[cols] + w == d[rows])                       # (float32 + float32)
        cand = np.append(np.where(ok, cols, NONE).astype(np.uint32), NONE)        # (+ a sentinel: reduceat needs valid starts)
        best = np.minimum.reduceat(cand, indptr[r0:r1] - lo)
        par[r0 - row_begin:r1 - row_begin] = np.where(lens > 0, best, NONE)
    dv = d[row_begin:row_end]
    v = np.arange(row_begin, row_end, dtype=np.int64)
    par = np.where(v == source, np.uint32(source), np.where(dv >= unreached, NONE, par)).astype(np.uint32)
    return par, int(np.count_nonzero((dv < unreached) & (v != source) & (par == NONE)))


def distances_by_definition(indptr, indices, data, source, num_iterations, unreached=INF):
    """Synchronous (min,+) iteration in float32 (numpy): d0 = unreached everywhere and 0 on the source,
    d_{k+1}[v] = min(unreached, min over the entries A[v, u] of fl(w + d_k[u])).  Returns (d after num_iterations, the first
    iteration that changed nothing -- num_iterations + 1 if every one changed something)."""
    indptr = np.asarray(indptr).astype(np.int64)
    n = indptr.shape[0] - 1
    cols = np.asarray(indices).astype(np.int64)
    w = np.asarray(data, dtype=np.float32)
    lens = np.diff(indptr)
    unreached = np.float32(unreached)
    d = np.full(max(n, int(cols.max(initial=0)) + 1), unreached, dtype=np.float32)
    d[source] = 0
    settled = num_iterations + 1
    for it in range(1, num_iterations + 1):
        cand = np.append(w + d[cols], unreached)
        new = d.copy()
        new[:n] = np.where(lens > 0, np.minimum(np.minimum.reduceat(cand, indptr[:n]), unreached), unreached)
        if np.array_equal(new, d):
            settled = min(settled, it)
        d = new
    return d, settled


def weights(kind, nnz, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 9, size=nnz)
    if kind == "int":
        return k.astype(np.float32)                                   # small integers: many equal-length paths
    return (k / 1024 + 1e-3 * rng.random(nnz)).astype(np.float32)     # no two paths of equal length


def raw_graph(name):
    return {"uniform_3000": lambda: datasets.uniform(3000, 4, seed=5),
            "rmat_4000": lambda: datasets.rmat(4000, 30000, seed=6),
            "rmat_sym_4000": lambda: datasets.rmat(4000, 40000, seed=8, symmetric=True),
            "rmat_sym_6016": lambda: datasets.rmat(6016, 90000, seed=21, symmetric=True)}[name]()


@functools.lru_cache(maxsize=None)
def weighted_graph(name, kind):
    """The raw weighted matrix (what a driver is given) -- shared, never modified"""
    m = raw_graph(name)
    m.adj_data = weights(kind, m.nnz, 100 + GRAPHS.index(name))
    return m


@functools.lru_cache(maxsize=None)
def prepared_graph(name, kind):
    """... and what the weighted SSSP driver makes of it: a weight-0 diagonal, padded to 128 (the oracle's container)"""
    m = weighted_graph(name, kind).copy()
    io.sssp_zero_diagonal(m)
    om = O.CSR(m.num_rows, m.num_cols, m.adj_data, m.adj_indices, m.adj_indptr)
    O.util_round_csr_matrix_dim(om, 128, 128)
    return om


# 0 and one more source per graph: a vertex from which the search reaches as many vertices as from 0 but needs more rounds, so
# that five iterations leave it visibly unfinished (chosen on the numpy definition alone: 7-12 rounds from 0, 8-14 from these)
SOURCES = {"uniform_3000": [0, 1], "rmat_4000": [0, 2000], "rmat_sym_4000": [0, 1], "rmat_sym_6016": [0, 1]}


def sources(name):
    return SOURCES[name]


@functools.lru_cache(maxsize=None)
def reference(name, kind, source, iters):
    """(distances, parents, orphans) by the definition on the prepared matrix -- shared, never modified"""
    om = prepared_graph(name, kind)
    d, _ = distances_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, source, iters)
    par, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d, source)
    return d, par, orphans


def test_library_exports_and_binds_gl_sssp_parents():
    L = capi.lib()
    for sym in ("gl_sssp_parents", "gl_sssp_parents_entries"):
        assert hasattr(L, sym), "libgraphlily_hip.so does not export %s" % sym
        assert sym in capi.EXPORTS
    assert L.gl_sssp_parents.argtypes is not None and len(L.gl_sssp_parents.argtypes) == 6
    assert L.gl_sssp_parents_entries.argtypes is not None and len(L.gl_sssp_parents_entries.argtypes) == 6
    for cls, names in ((capi.SpMSpVPlan, ("sssp_parents", "sssp_parents_entries")), (M.SpMSpVModule, ("sssp_parents",)),
                       (app.SSSP, ("parents",)), (io, ("sssp_zero_diagonal",)), (app, ("validate_sssp_tree",))):
        for name in names:
            assert callable(getattr(cls, name))
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "graphlily_hip.h")).read())
    assert ("int gl_sssp_parents(gl_spmspv_plan plan, const float *d_distance, float unreached, uint32_t source, "
            "uint32_t *d_parent, uint32_t *d_orphans /* may be NULL */);") in header
    assert ("int gl_sssp_parents_entries(gl_spmspv_plan plan, const float *d_distance, float unreached, uint32_t source, "
            "uint32_t *d_parent, uint64_t *entries_read);") in header


def test_compute_entry_point_fails_loudly_without_a_gpu():
    assert hasattr(capi.lib(), "gl_sssp_parents")
    if capi.device_count() == 0:
        rc = capi.lib().gl_sssp_parents(None, None, 1e9, 0, None, None)
        assert rc == capi.GL_ERR_NOT_INITIALIZED
        assert capi.lib().gl_sssp_parents_entries(None, None, 1e9, 0, None, None) == capi.GL_ERR_NOT_INITIALIZED


def _csr(rows):
    """rows: a list of [(column, weight), ...] in storage order"""
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    flat = [e for r in rows for e in r]
    return io.CSRMatrix(len(rows), len(rows), [e[1] for e in flat], [e[0] for e in flat], indptr)


def _rows_of(m):
    ip = m.adj_indptr.astype(np.int64)
    return [list(zip(m.adj_indices[ip[r]:ip[r + 1]].tolist(), m.adj_data[ip[r]:ip[r + 1]].tolist())) for r in range(m.num_rows)]


def test_zero_diagonal_keeps_weights_and_places_one_diagonal_entry_per_row():
    m = _csr([[(0, 5.0), (2, 1.5)],                 # diagonal present, first
              [(0, 2.0), (2, 3.0)],                 # absent: goes between 0 and 2
              [],                                   # empty row
              [(0, 1.0), (1, 2.0), (2, 0.25)],      # absent: goes last
              [(4, 7.0), (4, 8.0), (5, 1.0)],       # diagonal stored twice
              [(5, 0.0), (1, 4.0)]])                # columns do not ascend; the diagonal is kept where it is
    io.sssp_zero_diagonal(m)
    assert _rows_of(m) == [[(0, 0.0), (2, 1.5)], [(0, 2.0), (1, 0.0), (2, 3.0)], [(2, 0.0)], [(0, 1.0), (1, 2.0), (2, 0.25), (3, 0.0)],
                           [(4, 0.0), (5, 1.0)], [(5, 0.0), (1, 4.0)]]
    assert m.adj_indptr.dtype == np.uint32 and m.adj_indices.dtype == np.uint32 and m.adj_data.dtype == np.float32
    assert m.adj_indptr.tolist() == [0, 2, 5, 6, 10, 12, 14]
    before = _rows_of(m)
    io.sssp_zero_diagonal(m)                        # idempotent
    assert _rows_of(m) == before
    for name in GRAPHS[:2]:
        raw = weighted_graph(name, "float")
        m = raw.copy()
        io.sssp_zero_diagonal(m)
        ip = m.adj_indptr.astype(np.int64)
        rows = np.repeat(np.arange(m.num_rows), np.diff(ip))
        on_diag = m.adj_indices == rows
        assert np.array_equal(np.bincount(rows[on_diag], minlength=m.num_rows), np.ones(m.num_rows, np.int64))
        assert np.all(m.adj_data[on_diag] == 0)
        # everything else is the raw matrix, in its order
        rip = raw.adj_indptr.astype(np.int64)
        rrows = np.repeat(np.arange(raw.num_rows), np.diff(rip))
        keep = raw.adj_indices != rrows
        assert np.array_equal(m.adj_indices[~on_diag], raw.adj_indices[keep]) and np.array_equal(m.adj_data[~on_diag], raw.adj_data[keep])
        assert np.array_equal(rows[~on_diag], rrows[keep])
        asc = np.ones(m.nnz, bool)
        asc[1:] = (m.adj_indices[1:].astype(np.int64) > m.adj_indices[:-1]) | (rows[1:] != rows[:-1])
        rasc = np.ones(raw.nnz, bool)
        rasc[1:] = (raw.adj_indices[1:].astype(np.int64) > raw.adj_indices[:-1]) | (rrows[1:] != rrows[:-1])
        assert rasc.all() and asc.all(), "ascending rows stay ascending"


@pytest.mark.parametrize("bad", [-1.0, float("nan"), 1e9])
def test_zero_diagonal_rejects(bad):
    m = _csr([[(1, 1.0)], [(0, bad)], [(1, 2.0)]])
    with pytest.raises(ValueError, match="weight"):
        io.sssp_zero_diagonal(m)
    assert m.nnz == 3, "a refused matrix is left alone"


def test_zero_diagonal_refuses_more_rows_than_columns():
    m = io.CSRMatrix(3, 2, [1.0], [0], [0, 1, 1, 1])
    with pytest.raises(ValueError):
        io.sssp_zero_diagonal(m)


def test_unit_weights_give_the_oracles_distances():
    raw = raw_graph("uniform_3000")
    ip = raw.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(raw.num_rows), np.diff(ip))
    keep = raw.adj_indices != rows                  # no diagonal entries: every row gets one inserted
    m = io.CSRMatrix(raw.num_rows, raw.num_cols, np.ones(int(keep.sum()), np.float32), raw.adj_indices[keep],
                     np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=raw.num_rows))]))
    io.sssp_zero_diagonal(m)
    assert m.nnz == int(keep.sum()) + m.num_rows
    om = O.CSR(m.num_rows, m.num_cols, m.adj_data, m.adj_indices, m.adj_indptr)
    for source in (0, 1234):
        d, settled = distances_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, source, ITERS)
        assert settled <= ITERS
        assert np.array_equal(d, O.sssp(om, source, ITERS, M.FLOAT_INF))
        assert np.count_nonzero(d < INF) > 1000


def _line8(golden_dir):
    m = io.load_csr_matrix_from_float_npz(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert m.adj_indices.tolist() == list(range(7))                              # row v holds column v - 1: a chain from vertex 0
    m.adj_data = np.arange(1, 8, dtype=np.float32)
    d = np.array([0, 1, 3, 6, 10, 15, 21, 28], dtype=np.float32)
    p = np.array([0, 0, 1, 2, 3, 4, 5, 6], dtype=np.uint32)
    return m, d, p


def test_validator_accepts_a_hand_made_tree(golden_dir):
    m, d, p = _line8(golden_dir)
    assert app.validate_sssp_tree(m, 0, d, p) == 8
    assert app.validate_sssp_tree(m, 0, d, p, converged=False) == 8
    got, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, 0)
    assert np.array_equal(got, p) and orphans == 0
    prepared = m.copy()
    io.sssp_zero_diagonal(prepared)
    dd, settled = distances_by_definition(prepared.adj_indptr, prepared.adj_indices, prepared.adj_data, 0, 10)
    assert np.array_equal(dd, d) and settled == 8             # one more vertex per iteration, the eighth changes nothing
    assert app.validate_sssp_tree(prepared, 0, d, p) == 8     # (the weight-0 diagonal never objects)
    # three vertices reached, the rest not
    d3, p3 = d.copy(), p.copy()
    d3[3:], p3[3:] = INF, NONE
    assert app.validate_sssp_tree(m, 0, d3, p3, converged=False) == 3
    with pytest.raises(ValueError, match=r"\(rule 4\)"):
        app.validate_sssp_tree(m, 0, d3, p3)                   # A[3, 2] would reach vertex 3


def _diamond():
    """0 -> 1 -> 2 -> 3 -> 4 -> 5 -> 6 -> 7 with weights 1..7 and the shortcut A[5, 3] = 9: vertex 5 is reached at 15 both ways"""
    rows = [[], [(0, 1.0)], [(1, 2.0)], [(2, 3.0)], [(3, 4.0)], [(3, 9.0), (4, 5.0)], [(5, 6.0)], [(6, 7.0)]]
    d = np.array([0, 1, 3, 6, 10, 15, 21, 28], dtype=np.float32)
    p = np.array([0, 0, 1, 2, 3, 3, 5, 6], dtype=np.uint32)    # 5: the smaller of its two tight predecessors
    return rows, d, p


@pytest.mark.parametrize("what,rule", [("source is not its own parent", 1), ("source at a distance", 1), ("reached vertex without parent", 2),
                                       ("unreached vertex with a parent", 2), ("parent is no vertex", 3), ("parent is not an entry", 3),
                                       ("right entry, wrong sum", 3), ("equal-distance parent through a weight-0 entry", 3),
                                       ("a shorter way was left unused", 4)])
def test_validator_rejects(what, rule):
    rows, d, p = _diamond()
    m = _csr(rows)
    assert app.validate_sssp_tree(m, 0, d, p) == 8
    got, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, 0)
    assert np.array_equal(got, p) and orphans == 0
    p54 = p.copy()
    p54[5] = 4
    assert app.validate_sssp_tree(m, 0, d, p54) == 8          # the other tight predecessor: a valid tree, not the canonical one
    converged = True
    if what == "source is not its own parent":
        p[0] = 1
    elif what == "source at a distance":
        d[0] = 0.5
    elif what == "reached vertex without parent":
        p[6] = NONE
    elif what == "unreached vertex with a parent":
        d[7] = INF
    elif what == "parent is no vertex":
        p[6] = 8
    elif what == "parent is not an entry":
        p[6] = 4                        # nearer than vertex 6, but A[6, 4] is no entry
    elif what == "right entry, wrong sum":
        rows[5][0] = (3, 8.0)           # 5 is now reached at 14 through 3; A[5, 4] is an entry, but 10 + 5 is 15
        m = _csr(rows)
        d[5:] = [14, 20, 27]
        assert app.validate_sssp_tree(m, 0, d, p) == 8
        p[5] = 4
    elif what == "equal-distance parent through a weight-0 entry":
        rows[5][1] = (4, 0.0)           # 5 sits at 10 like 4: the entry A[5, 4] is tight, but 4 is no nearer
        m = _csr(rows)
        d[5:] = [10, 16, 23]
        p[5] = 4
        want, orphans = parents_by_definition(m.adj_indptr, m.adj_indices, m.adj_data, d, 0)
        assert want[5] == NONE and orphans == 1, "by the definition vertex 5 is an orphan"
        converged = False
    else:
        rows[5][0] = (3, 8.0)           # the tree through 4 obeys rules 1-3, but A[5, 3] gives 14
        m = _csr(rows)
        p[5] = 4
        assert app.validate_sssp_tree(m, 0, d, p, converged=False) == 8          # rule 4 is skipped on request
    with pytest.raises(ValueError, match=r"\(rule %d\)" % rule):
        app.validate_sssp_tree(m, 0, d, p, converged=converged)


@pytest.mark.parametrize("kind", WEIGHTINGS)
@pytest.mark.parametrize("name", GRAPHS)
def test_definition_agrees_with_the_validator_on_random_graphs(name, kind):
    om = prepared_graph(name, kind)
    rng = np.random.default_rng(1)
    ip = om.adj_indptr.astype(np.int64)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(ip[:-1], ip[1:])]).astype(np.int64)
    for source in sources(name):
        d, settled = distances_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, source, ITERS)
        assert settled <= ITERS, "converged inside the %d iterations" % ITERS
        assert np.array_equal(d, O.sssp(om, source, ITERS, M.FLOAT_INF))
        par, orphans = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d, source)
        reached = int(np.count_nonzero(d < INF))
        assert orphans == 0 and par[source] == source and 2000 < reached
        assert app.validate_sssp_tree(om, source, d, par) == reached
        # ties: vertices with more than one tight predecessor (the minimum decides) -- integer weights have them
        rows = np.repeat(np.arange(om.num_rows), np.diff(ip))
        cols = om.adj_indices.astype(np.int64)
        tight = (d[cols] < d[rows]) & (d[cols] + om.adj_data == d[rows])
        tied = int(np.count_nonzero(np.bincount(rows[tight], minlength=om.num_rows) > 1))
        assert (tied > 100) if kind == "int" else (tied == 0)
        # the order of a row's entries does not matter
        par2, _ = parents_by_definition(om.adj_indptr, om.adj_indices[perm], om.adj_data[perm], d, source)
        assert np.array_equal(par, par2)
        # row ranges give slices
        mid = om.num_rows // 3
        a, oa = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d, source, INF, 0, mid)
        b, ob = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d, source, INF, mid, om.num_rows)
        assert np.array_equal(np.concatenate([a, b]), par) and oa + ob == 0
        # a damaged tree does not pass
        kids = np.flatnonzero((d < INF) & (d > 0))
        bad = par.copy()
        bad[kids[-1]] = kids[-1]
        with pytest.raises(ValueError, match=r"\(rule 3\)"):
            app.validate_sssp_tree(om, source, d, bad)
        bad = par.copy()
        bad[kids[0]] = NONE
        with pytest.raises(ValueError, match=r"\(rule 2\)"):
            app.validate_sssp_tree(om, source, d, bad)
        # cut short: some vertices' predecessors have moved on since -- orphans, which the validator reports under rule 2
        d5, _ = distances_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, source, SHORT)
        assert np.array_equal(d5, O.sssp(om, source, SHORT, M.FLOAT_INF))
        par5, orphans5 = parents_by_definition(om.adj_indptr, om.adj_indices, om.adj_data, d5, source)
        assert orphans5 > 0 and orphans5 == np.count_nonzero((d5 < INF) & (par5 == NONE))
        with pytest.raises(ValueError, match=r"\(rule 2\)"):
            app.validate_sssp_tree(om, source, d5, par5, converged=False)


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("sssp_parents_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([SSSP_DRIVER, str(tmp_path / "none.npz"), str(tmp_path), "0", "4"], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
