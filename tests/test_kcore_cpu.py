"""CPU suite of the k-core decomposition (gl_kcore, SpMVPlan.kcore, SpMVModule.kcore, io.symmetrize_simple, app.KCore,
app.validate_cores): the export and its bindings exist, the preparation gives a symmetric, sorted, simple matrix, the host-side
validator accepts networkx's core numbers and refuses one violation per rule, the driver refuses what it cannot do, and the C++
driver compiles against include/ and symmetrises like the Python function.  tests/test_gpu_kcore.py compares the kernels with
core_numbers_by_peeling (kept here) bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver, named_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCORE_DRIVER = os.path.join(ROOT, "build", "kcore_driver")
DECL = "int gl_kcore(gl_spmv_plan plan, uint32_t *d_core, uint32_t *d_order /* may be NULL */, uint32_t *h_stats /* may be NULL, 4 words */);"
# degeneracy and sum of the core numbers of the graphs padded to 128: computed on the CPU by networkx.core_number (3.4.2) and by a
# numpy peel, which agree on all four; test_validate_cores_accepts_networkx recomputes the first two with networkx every time
RECORDS = {"uniform_10K_10": (15, 149296), "rmat_20K": (147, 359200), "rmat_sym_50K": (177, 721295), "gplus_small": (355, 1055136)}


def _csr(n, rows, cols, data=None, num_cols=None):
    """entries in the order given inside a row (np.argsort stable by row): duplicates and unsorted columns stay as they are"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    data = np.ones(rows.shape[0], np.float32) if data is None else np.asarray(data, np.float32)[order]
    return io.CSRMatrix(n, n if num_cols is None else num_cols, data, cols.astype(np.uint32), np.cumsum(indptr).astype(np.uint32))


def core_numbers_by_peeling(sym):
    """The definition, one vertex at a time (Batagelj & Zaversnik's bucket order, written with a heap): repeatedly remove a
    vertex of the smallest remaining degree; core[v] = the largest such degree seen up to v's removal.  -> (core as uint32[n],
    the removal order as uint32[n]).  `sym` is a symmetric simple CSRMatrix (io.symmetrize_simple)."""
    import heapq
    n = sym.num_rows
    ip, idx = sym.adj_indptr.astype(np.int64).tolist(), sym.adj_indices.astype(np.int64).tolist()
    deg = [ip[v + 1] - ip[v] for v in range(n)]
    heap = [(d, v) for v, d in enumerate(deg)]
    heapq.heapify(heap)
    core, order, gone, k = np.zeros(n, np.uint32), [], [False] * n, 0
    while heap:
        d, v = heapq.heappop(heap)
        if gone[v] or d != deg[v]:
            continue
        k = max(k, d)
        core[v], gone[v] = k, True
        order.append(v)
        for u in idx[ip[v]:ip[v + 1]]:
            if not gone[u]:
                deg[u] -= 1
                heapq.heappush(heap, (deg[u], u))
    return core, np.array(order, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def prepared(name):
    """-> (the matrix as given, padded to 128, its symmetric simple form, core numbers of the padded matrix's vertices, a
    degeneracy ordering); computed once and shared, never written"""
    from test_cc_cpu import many_components
    if name in ("line_8", "eye_10"):
        raw = io.load_csr_matrix_from_float_npz(os.path.join(ROOT, "tests", "golden", name + "_csr_float32.npz"))
    elif name == "many":
        raw = many_components()
    else:
        raw = named_matrix(name)
    m = raw.copy()
    io.util_round_csr_matrix_dim(m, 128, 128)
    sym, _ = io.symmetrize_simple(m)
    core, order = core_numbers_by_peeling(sym)
    core.setflags(write=False)
    order.setflags(write=False)
    if name in RECORDS:
        assert (int(core.max()), int(core.sum())) == RECORDS[name]
    return raw, m, sym, core, order


# sub-rounds of the same four graphs: the schedule of DESIGN.md 4.14 replayed on the host a whole launch at a time (EXPERIMENTS.md
# Round 13).  The isolated padding vertices of level 0 are a sub-round; the slice that completes the queue is never peeled.
SUB_ROUNDS = {"uniform_10K_10": 21, "rmat_20K": 396, "rmat_sym_50K": 486, "gplus_small": 504}


def _nx_core_numbers(sym):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(sym.num_rows))
    rows = np.repeat(np.arange(sym.num_rows), np.diff(sym.adj_indptr.astype(np.int64)))
    G.add_edges_from(zip(rows.tolist(), sym.adj_indices.tolist()))
    want = nx.core_number(G)
    return np.array([want[v] for v in range(sym.num_rows)], dtype=np.uint32)


def test_library_exports_and_binds_the_entry_point():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "graphlily_hip.h")).read()
    assert hasattr(L, "gl_kcore"), "libgraphlily_hip.so does not export gl_kcore"
    assert "gl_kcore" in capi.EXPORTS and len(L.gl_kcore.argtypes) == 4
    assert DECL in header
    assert callable(capi.SpMVPlan.kcore) and callable(M.SpMVModule.kcore) and callable(io.symmetrize_simple)
    assert callable(app.KCore.run) and callable(app.KCore.k_core) and callable(app.validate_cores)
    assert "kcore(DeviceBuffer core, uint32_t *order = nullptr, uint32_t *stats = nullptr)" in open(
        os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    kcore_h = open(os.path.join(ROOT, "include", "graphlily", "app", "kcore.h")).read()
    for piece in ("class KCore", "run(bool want_order = false)", "degeneracy()", "core_sizes()", "util_symmetrize_simple"):
        assert piece in kcore_h
    assert "util_symmetrize_simple" in open(os.path.join(ROOT, "include", "graphlily", "io", "data_formatter.h")).read()
    assert "gl_kcore.hip" in open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_kcore(None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


def _hand_made():
    """6 x 9: a duplicate, a diagonal entry, a zero-valued entry that is the only copy of its edge, a zero-valued entry next to a
    live copy, one-way entries, unsorted columns, a column beyond the rows"""
    rows = [0, 0, 0, 0, 1, 2, 2, 3, 3, 5, 5]
    cols = [3, 1, 1, 0, 4, 0, 5, 2, 0, 8, 2]
    data = [1, 2, 1, 7, 0, 0, 3, 1, 1, 1, 0]
    return _csr(6, rows, cols, data, num_cols=9)


def test_symmetrize_simple_on_hand_made_matrices():
    m = _hand_made()
    before = (m.adj_indptr.copy(), m.adj_indices.copy(), m.adj_data.copy())
    s, deg = io.symmetrize_simple(m)
    assert all(np.array_equal(a, b) for a, b in zip(before, (m.adj_indptr, m.adj_indices, m.adj_data))), "the input is left alone"
    # edges: {0,3} (stored both ways), {0,1} (twice one way), {2,5} (one live copy), {2,3}, {5,8}; (1,4) and (2,0) are zero-valued
    want = {0: [1, 3], 1: [0], 2: [3, 5], 3: [0, 2], 4: [], 5: [2, 8], 6: [], 7: [], 8: [5]}
    assert (s.num_rows, s.num_cols) == (9, 9) and s.adj_indptr.dtype == np.uint32 and s.adj_indices.dtype == np.uint32
    ip = s.adj_indptr.astype(np.int64)
    assert {v: s.adj_indices[ip[v]:ip[v + 1]].tolist() for v in range(9)} == want
    assert s.adj_data.dtype == np.float32 and np.all(s.adj_data == 1) and s.nnz == 10
    assert deg.dtype == np.uint32 and np.array_equal(deg, np.diff(ip))
    e = _csr(4, [], [])
    s, deg = io.symmetrize_simple(e)
    assert s.nnz == 0 and np.array_equal(s.adj_indptr, np.zeros(5, np.uint32)) and not deg.any()
    d = _csr(4, [0, 1, 2], [0, 1, 2], [1, 0, 5])                     # only a diagonal
    assert io.symmetrize_simple(d)[0].nnz == 0


@pytest.mark.parametrize("graph", ["uniform_10K_10", "rmat_20K", "many"])
def test_symmetrize_simple_is_symmetric_sorted_and_simple(graph):
    import scipy.sparse as sp
    _, m, s, _, _ = prepared(graph)
    n = max(m.num_rows, m.num_cols)
    ip = s.adj_indptr.astype(np.int64)
    rows, cols = np.repeat(np.arange(n), np.diff(ip)), s.adj_indices.astype(np.int64)
    inside = np.ones(cols.shape[0], bool)
    inside[ip[:-1][np.diff(ip) > 0]] = False                         # (the first entry of every non-empty row)
    assert np.all(cols[1:][inside[1:]] > cols[:-1][inside[1:]]), "rows are strictly ascending"
    assert not np.any(rows == cols)
    S = sp.csr_matrix((np.ones(s.nnz, np.int64), cols, ip), shape=(n, n))
    assert (S != S.T).nnz == 0
    A = sp.csr_matrix((m.adj_data[:m.nnz] != 0, m.adj_indices[:m.nnz].astype(np.int64), m.adj_indptr.astype(np.int64)), shape=(m.num_rows, m.num_cols))
    A.resize((n, n))
    A.eliminate_zeros()
    W = (A + A.T).tocsr()
    W.setdiag(False)
    W.eliminate_zeros()
    assert ((W != 0) != (S != 0)).nnz == 0, "exactly the edges of the matrix"
    assert np.array_equal(io.symmetrize_simple(m)[1], np.diff(ip))
    assert np.array_equal(io.symmetrize_simple(s)[0].adj_indices, s.adj_indices), "idempotent"


def test_symmetrize_simple_refuses_more_entries_than_32_bit_offsets(monkeypatch):
    """as triangle_orient does; the count is faked (5e9 entries are not built here): np.cumsum is what fills the offsets"""
    m = _hand_made()
    real = np.cumsum

    def huge(a, out=None, **kw):
        r = real(a, out=out, **kw)
        if out is not None:
            out[-1] = 5_000_000_000
        return r
    monkeypatch.setattr(np, "cumsum", huge)
    with pytest.raises(ValueError, match="symmetrize_simple: 5000000000 entries do not fit 32-bit offsets"):
        io.symmetrize_simple(m)


@pytest.mark.parametrize("graph", ["uniform_10K_10", "rmat_20K"])
def test_validate_cores_accepts_networkx(graph):
    raw, m, s, core, order = prepared(graph)
    want = _nx_core_numbers(s)
    assert np.array_equal(core, want)
    assert (int(want.max()), int(want.sum())) == RECORDS[graph]
    assert app.validate_cores(m, want) == RECORDS[graph][0]
    assert app.validate_cores(raw, want) == RECORDS[graph][0]        # (an array longer than the matrix: the drivers pad)
    assert app.validate_cores(m, want, order) == RECORDS[graph][0]
    assert app.validate_cores(s, np.concatenate([want, np.zeros(64, np.uint32)]),
                              np.concatenate([np.arange(s.num_rows, s.num_rows + 64, dtype=np.uint32), order])) == RECORDS[graph][0]


def test_validate_cores_refuses_one_violation_per_rule():
    _, m, s, core, order = prepared("uniform_10K_10")
    ip = s.adj_indptr.astype(np.int64)
    deg = np.diff(ip)
    with pytest.raises(ValueError, match="core numbers for a"):
        app.validate_cores(m, core[:100])
    # rule 1: a value too high -- above the degree, and within the degree but without the neighbours to hold it
    v = int(np.flatnonzero(core == deg)[0])
    bad = core.copy()
    bad[v] += 1
    with pytest.raises(ValueError, match=r"vertex %d of degree %d is given core number %d \(rule 1\)" % (v, deg[v], bad[v])):
        app.validate_cores(m, bad)
    v = int(np.flatnonzero((core < deg) & (core == core.max()))[0])
    bad = core.copy()
    bad[v] += 1
    with pytest.raises(ValueError, match=r"vertex %d is given core number %d, but only \d+ of its neighbours have one that high \(rule 1\)" % (v, bad[v])):
        app.validate_cores(m, bad)
    # rule 2: a value too low passes rule 1 (fewer neighbours are asked for) and is caught by the independent computation
    v = int(np.flatnonzero(core == core.max())[3])
    bad = core.copy()
    bad[v] -= 1
    with pytest.raises(ValueError, match=r"vertex %d is given core number %d, its core number is %d \(rule 2\)" % (v, bad[v], core[v])):
        app.validate_cores(m, bad)
    low = np.minimum(core, 3)                                         # (every vertex at most 3: rule 1 holds everywhere)
    with pytest.raises(ValueError, match=r"rule 2"):
        app.validate_cores(m, low)
    # rule 3: a vertex moved to the front of its core-number class has all its neighbours of that class and above behind it
    k = int(core.max())
    first = int(np.flatnonzero(core[order] == k)[0])
    pos = np.empty(order.shape[0], np.int64)
    pos[order] = np.arange(order.shape[0])
    rows = np.repeat(np.arange(s.num_rows), deg)
    behind = np.bincount(rows[pos[s.adj_indices] > pos[rows]], minlength=s.num_rows)
    assert np.all(behind <= core)
    # a swap of the class's first vertex f with a later vertex w of the class, chosen so that w then has too many behind it
    cls = order[first:]
    ahead_in_class = np.bincount(rows[(pos[s.adj_indices] >= first) & (pos[s.adj_indices] < pos[rows])], minlength=s.num_rows)
    w = int(cls[np.argmax((behind + ahead_in_class)[cls] > k)])
    assert (behind + ahead_in_class)[w] > k and pos[w] > first
    swapped = order.copy()
    swapped[first], swapped[pos[w]] = order[pos[w]], order[first]
    with pytest.raises(ValueError, match=r"vertex %d with core number %d has \d+ neighbours behind it in the order \(rule 3\)" % (w, k)):
        app.validate_cores(m, core, swapped)
    with pytest.raises(ValueError, match=r"core number \d+\) before vertex \d+ \(core number \d+\) \(rule 3\)"):
        app.validate_cores(m, core, order[::-1].copy())
    twice = order.copy()
    twice[5] = twice[6]
    with pytest.raises(ValueError, match=r"no permutation: vertex %d occurs" % min(int(order[5]), int(order[6]))):
        app.validate_cores(m, core, twice)
    with pytest.raises(ValueError, match=r"an order of 10 vertices"):
        app.validate_cores(m, core, order[:10])


def test_host_peel_of_the_validator_agrees_on_closed_forms():
    """app._core_numbers_of (sets per level, numpy) against the one-vertex-at-a-time definition kept in this file"""
    for name in ("many", "line_8", "eye_10"):
        _, m, s, core, order = prepared(name)
        assert np.array_equal(app._core_numbers_of(s.adj_indptr, s.adj_indices, s.num_rows), core)
        assert app.validate_cores(m, core, order) == int(core.max())
    _, _, s, core, _ = prepared("many")
    assert int(core.max()) == 2 and set(np.unique(core).tolist()) == {0, 1, 2}     # padding, paths and stars, cycles


class _TwoRanks:
    """what the drivers ask of a communicator, claiming rank 0 of 2"""
    rank, world_size, distributed = 0, 2, True


def test_driver_refuses_row_shards_and_a_run_before_send(golden_dir):
    with pytest.raises(NotImplementedError, match="row shards"):
        app.KCore(comm=_TwoRanks(), backend=CpuBackend())
    kc = app.KCore(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        kc.run()
    kc.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (kc.n_, kc.n_real_) == (128, 8) and kc.degrees_.shape == (128,) and kc.degrees_[:8].max() == 2 and not kc.degrees_[8:].any()
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        kc.run(order=True)
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        kc.k_core(1)


def test_cpp_driver_compiles_symmetrizes_alike_and_fails_loudly_without_gpu(tmp_path):
    import scipy.sparse as sp
    build_cpp_driver("kcore_driver.cpp")
    m = _hand_made()
    A = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int32), m.adj_indptr.astype(np.int32)), shape=(m.num_rows, m.num_cols), dtype=np.float32)
    path = str(tmp_path / "hand_made_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    r = subprocess.run([KCORE_DRIVER, "--symmetrize", path], capture_output=True, text=True, timeout=120)     # host only
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {line.split(":")[0]: line.split(":")[1].split() for line in r.stdout.splitlines() if ":" in line}
    p = m.copy()
    io.util_round_csr_matrix_dim(p, 128, 128)
    s, deg = io.symmetrize_simple(p)
    assert [int(x) for x in got["shape"]] == [s.num_rows, s.num_cols] == [128, 128]
    assert np.array_equal(np.array(got["indptr"], dtype=np.uint32), s.adj_indptr)
    assert np.array_equal(np.array(got["indices"], dtype=np.uint32), s.adj_indices)
    assert np.array_equal(np.array(got["data"], dtype=np.float32), s.adj_data)
    assert np.array_equal(np.array(got["degrees"], dtype=np.uint32), deg)
    if capi.device_count() == 0:
        r = subprocess.run([KCORE_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
