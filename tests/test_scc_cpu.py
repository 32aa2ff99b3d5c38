"""CPU suite of the strongly connected components (gl_scc, SpMVPlan.scc, SpMVModule.scc, app.StronglyConnectedComponents,
app.validate_strong_components): the export and its bindings exist, the host model of the kernel's algorithm -- trim, forward,
backward, in synchronous rounds -- meets the closed forms and scipy's strong components on every named case, the labels do not
depend on the priorities while the passes may, the validator accepts the truth and refuses one violation per rule, the condensation
of a hand-made graph is the one worked out by hand, the driver prepares both patterns and refuses what it cannot do, and the C++
driver compiles against include/.  tests/test_gpu_scc.py compares the kernels with scc_model (kept here) on the cases of scc_case.

The model counts what the kernel reports: PASSES are the passes that reached the forward phase, TRIMMED the vertices the trim phase
removed over the whole run (both are functions of graph and priorities), ROUNDS the sweeps of all three phases, every phase's last
sweep, which changes nothing, included.  The device's rounds are at most the model's: it may see a word written earlier in the same
sweep, and it trims the vertices with an empty row before its first round."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver
from test_cc_cpu import permute_rows
from test_kcore_cpu import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCC_DRIVER = os.path.join(ROOT, "build", "scc_driver")
HEADER = "graphlily_hip_scc.h"
DECL = ("int gl_scc(gl_spmv_plan plan_in, gl_spmv_plan plan_out /* == plan_in: symmetric */, const uint32_t *d_prio /* may be NULL: all equal */, "
        "uint32_t *d_label, uint64_t *h_stats /* may be NULL, 5 words: components, passes, trimmed, rounds, launches */);")
N = 640                                     # every named case: 640 vertices, a multiple of the drivers' padding, at least 40 unused


# ------------------------------------------------------------------ the host model
def scc_model(n, src, dst, prio=None):
    """The algorithm of gl_scc.hip with synchronous rounds, on the edges src[i] -> dst[i] (simple: no loops, no duplicates) ->
    (labels uint32[n], components, passes, trimmed, rounds).  The key of a vertex: larger prio first, then the smaller vertex."""
    import scipy.sparse as sp
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    p = np.zeros(n, np.uint64) if prio is None else np.asarray(prio).astype(np.uint64)
    key = ((np.uint64(0xFFFFFFFF) - p) << np.uint64(32)) | np.arange(n, dtype=np.uint64)      # (64 bits, unsigned: the device's word)
    A = sp.csr_matrix((np.ones(src.shape[0]), (dst, src)), shape=(n, n))       # row v: the predecessors of v
    At = A.T.tocsr()                                                         # row v: its successors
    live, root = np.ones(n, bool), np.full(n, -1, np.int64)
    passes = trimmed = rounds = 0
    ident = np.arange(n)
    while live.any():
        while True:                                                          # trim
            rounds += 1
            x = live.astype(np.float64)
            gone = live & ((A @ x == 0) | (At @ x == 0))
            if not gone.any():
                break
            root[gone], live[gone] = ident[gone], False
            trimmed += int(gone.sum())
        if not live.any():
            break
        passes += 1
        e = live[src] & live[dst]
        s, d = src[e], dst[e]
        colkey = np.where(live, key, np.uint64(0xFFFFFFFFFFFFFFFF))
        while True:                                                          # forward: the best key over the live predecessors
            rounds += 1
            new = colkey.copy()
            np.minimum.at(new, d, colkey[s])
            if np.array_equal(new, colkey):
                break
            colkey = new
        col = (colkey & np.uint64(0xFFFFFFFF)).astype(np.int64)
        mark = live & (col == ident)
        inside = col[s] == col[d]
        s, d = s[inside], d[inside]
        while True:                                                          # backward: inside the colour class, towards the root
            rounds += 1
            add = np.zeros(n, bool)
            add[s[mark[d]]] = True
            add &= live & ~mark
            if not add.any():
                break
            mark |= add
        root[mark], live[mark] = col[mark], False
    lab = np.full(n, n, np.int64)
    np.minimum.at(lab, root, ident)
    lab = lab[root]
    return lab.astype(np.uint32), int(np.count_nonzero(lab == ident)), passes, trimmed, rounds


def scipy_labels(n, src, dst):
    """scipy's strong components, every class renamed to its smallest vertex -> (labels uint32[n], count)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.csr_matrix((np.ones(len(src)), (np.asarray(src, np.int64), np.asarray(dst, np.int64))), shape=(n, n))
    k, comp = connected_components(A, directed=True, connection="strong")
    smallest = np.full(k, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.uint32), int(k)


# ------------------------------------------------------------------ the named cases
def _rename(src, dst, used, seed):
    """the vertices 0 .. used - 1 scattered over 0 .. N - 1 by a seeded permutation -> (src, dst, where[used])"""
    where = np.random.default_rng(seed).permutation(N)[:used]
    return where[np.asarray(src, np.int64)], where[np.asarray(dst, np.int64)], where


def _chain(order):
    """two-cycles (order[2 i], order[2 i + 1]), each with a one-way edge to the next"""
    k = len(order) // 2
    s, d = [], []
    for i in range(k):
        a, b = order[2 * i], order[2 * i + 1]
        s += [a, b]
        d += [b, a]
        if i + 1 < k:
            s.append(b)
            d.append(order[2 * i + 2])
    return np.array(s), np.array(d)


def _cliques(k):
    """disjoint complete digraphs on k vertices, as many as fit 600, with one-way edges from every vertex of one to the same
    vertex of the next (so rows of the pattern have k - 1 or k entries)"""
    count = 600 // k
    i, j = np.divmod(np.arange(k * k), k)
    i, j = i[i != j], j[i != j]
    src = np.concatenate([c * k + i for c in range(count)] + [c * k + np.arange(k) for c in range(count - 1)])
    dst = np.concatenate([c * k + j for c in range(count)] + [(c + 1) * k + np.arange(k) for c in range(count - 1)])
    return src, dst, count


def _bowtie():
    """IN tree (vertices 0 .. 99, edges towards vertex 0's side: child -> parent), a core cycle 100 .. 299 entered from the
    tree's root, an OUT tree 300 .. 399 left from the core, tendrils (a path out of IN that never reaches the core, 400 .. 419,
    and a path into OUT from outside, 420 .. 439) and an isolated two-cycle 440, 441.  -> (src, dst, used, labels by construction)"""
    s, d = [], []
    for c in range(1, 100):                              # IN: every child points at its parent, so all of IN reaches vertex 0
        s.append(c), d.append((c - 1) // 2)
    s.append(0), d.append(100)
    core = np.arange(100, 300)
    s += core.tolist()
    d += np.roll(core, -1).tolist()
    s += [150, 250]                                      # two chords inside the core
    d += [120, 101]
    s.append(299), d.append(300)
    for c in range(1, 100):                              # OUT: every parent points at its children
        s.append(300 + (c - 1) // 2), d.append(300 + c)
    s.append(57), d.append(400)
    s += list(range(400, 419))
    d += list(range(401, 420))
    s += list(range(420, 439)) + [439]
    d += list(range(421, 440)) + [377]
    s += [440, 441]
    d += [441, 440]
    return np.array(s), np.array(d), 442


@functools.lru_cache(maxsize=None)
def _random_graphs():
    """ONE stream of default_rng(1), drawn from in this order: for (n, m) in (64, 100), (300, 500), (300, 1500), (1000, 1400) the m
    pairs, of which the unique non-loop ones are the edges, then a permutation of the n vertices as priorities.  The anchors of
    test_closed_forms_of_the_model (164, 3 and 704 components) belong to this stream."""
    rng = np.random.default_rng(1)
    out = {}
    for n, m in ((64, 100), (300, 500), (300, 1500), (1000, 1400)):
        e = np.unique(rng.integers(0, n, (m, 2)), axis=0)
        e = e[e[:, 0] != e[:, 1]]
        out["%d_%d" % (n, m)] = (e[:, 0], e[:, 1], rng.permutation(n).astype(np.uint32))
    return out


@functools.lru_cache(maxsize=None)
def scc_case(name):
    """-> (csr_in, csr_out or None, prio or None, (labels, components, passes, trimmed, rounds) of the model, (src, dst)): the
    patterns as io.simple_pattern prepares them on N vertices; read-only arrays, shared by both test files"""
    rng = np.random.default_rng(1)
    prio = None
    kind, _, arg = name.partition("_")
    if name == "cycle":
        s = np.arange(600)
        src, dst, _ = _rename(s, (s + 1) % 600, 600, 11)
    elif name == "path":
        s = np.arange(599)
        src, dst, _ = _rename(s, s + 1, 600, 12)
    elif name in ("chain_asc", "chain_desc", "chain_asc_prio"):
        order = np.arange(80) if name != "chain_desc" else np.arange(80)[::-1]
        src, dst = _chain(order)
        if name == "chain_asc_prio":                      # priorities descending along the chain: the LAST component is the best
            prio = np.zeros(N, np.uint32)
            prio[:80] = np.arange(1, 81)
    elif kind == "cliques":
        s, d, _ = _cliques(int(arg))
        src, dst, _ = _rename(s, d, 600, 13)
    elif kind == "dag":
        k = int(arg)
        i, j = np.divmod(np.arange(k * k), k)
        src, dst, _ = _rename(i[i < j], j[i < j], k, 14)
    elif name == "hub":
        leaves = np.arange(1, 601)
        src, dst, _ = _rename(np.concatenate([np.zeros(600, np.int64), leaves]), np.concatenate([leaves, np.zeros(600, np.int64)]), 601, 15)
    elif name == "bowtie":
        s, d, used = _bowtie()
        src, dst, _ = _rename(s, d, used, 16)
    elif kind == "random":
        n = int(arg.split("_")[0])
        src, dst, perm = _random_graphs()["_".join(arg.split("_")[:2])]
        if name.endswith("_perm"):
            prio = np.zeros(1024, np.uint32)
            prio[:n] = perm
    elif name == "symmetric":
        e = np.unique(rng.integers(0, 600, (450, 2)), axis=0)
        e = e[e[:, 0] != e[:, 1]]
        src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
        key = np.unique(src * N + dst)
        src, dst = key // N, key % N
    elif name == "empty":
        src = dst = np.zeros(0, np.int64)
    else:
        raise KeyError(name)
    n = N if kind != "random" or int(arg.split("_")[0]) <= N else 1024
    if prio is not None:
        prio = prio[:n]
        prio.setflags(write=False)
    cin, cout, _ = io.simple_pattern(_csr(n, dst, src))           # an entry A[v, u] is the edge u -> v
    if cout is None and name != "symmetric":                      # (hub: symmetric too, and still given as two plans)
        cout = cin.copy()
    want = scc_model(n, src, dst, prio)
    for m in (cin, cout):
        if m is not None:
            for arr in (m.adj_indptr, m.adj_indices, m.adj_data):
                arr.setflags(write=False)
    want[0].setflags(write=False)
    return cin, cout, prio, want, (src, dst)


CLIQUE_SIZES = (3, 17, 65, 130)
CASES = (["cycle", "path", "chain_asc", "chain_desc", "chain_asc_prio", "hub", "bowtie", "symmetric"]
         + ["cliques_%d" % k for k in CLIQUE_SIZES] + ["dag_%d" % k for k in CLIQUE_SIZES]
         + ["random_300_500", "random_300_1500", "random_1000_1400", "random_300_500_perm", "random_300_1500_perm", "random_1000_1400_perm"])


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_scc"), "libgraphlily_hip.so does not export gl_scc"
    assert len(L.gl_scc.argtypes) == 5
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_scc"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_scc" not in capi.EXPORTS and "gl_scc" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.scc) and callable(M.SpMVModule.scc)
    assert callable(app.StronglyConnectedComponents.run) and callable(app.StronglyConnectedComponents.condensation)
    assert callable(app.validate_strong_components)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void scc(SpMVModule *out, DeviceBuffer label, const uint32_t *prio = nullptr, uint64_t *stats = nullptr)" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    scc_h = open(os.path.join(ROOT, "include", "graphlily", "app", "scc.h")).read()
    for piece in ("class StronglyConnectedComponents : public app::PatternApp", "prepare(", "run(", "labels()", "num_components()",
                  "largest_component()", "component_sizes()", "is_dag()", "passes()", "trimmed()", "rounds()", "launches()",
                  "util_simple_pattern", "util_coloring_priorities"):
        assert piece in scc_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_scc.hip" in make and HEADER in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "scc_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_scc(None, None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


@pytest.mark.parametrize("name", CASES)
def test_model_equals_scipy_on_every_case(name):
    cin, cout, prio, (lab, comps, passes, trimmed, rounds), (src, dst) = scc_case(name)
    n = cin.num_rows
    want, k = scipy_labels(n, src, dst)
    assert np.array_equal(lab, want) and comps == k
    assert app.validate_strong_components(cin, lab) == k
    assert passes <= k - trimmed                                         # a pass removes at least one component, trim exactly one each
    assert rounds >= passes and trimmed <= n
    assert (cout is None) == (name == "symmetric")


def test_closed_forms_of_the_model():
    lab, comps, passes, trimmed, _ = scc_case("cycle")[3]
    members = np.flatnonzero(np.bincount(lab, minlength=N)[lab] == 600)
    assert members.shape[0] == 600 and np.all(lab[members] == members.min())
    assert (comps, passes, trimmed) == (1 + 40, 1, 40)                  # the 40 unused vertices are trimmed, the cycle is one pass
    lab, comps, passes, trimmed, rounds = scc_case("path")[3]
    assert np.array_equal(lab, np.arange(N)) and (comps, passes, trimmed) == (N, 0, N)
    assert rounds == 301                                                 # both ends at once, and the last round removes nothing
    for name, p in (("chain_asc", 40), ("chain_desc", 1), ("chain_asc_prio", 1)):       # the documented worst case, pinned
        lab, comps, passes, trimmed, _ = scc_case(name)[3]
        assert passes == p and comps - (N - 80) == 40 and trimmed == N - 80, name
        assert np.array_equal(lab[:80], np.arange(80) // 2 * 2)
    for k in CLIQUE_SIZES:
        cin, cout, _, (lab, comps, passes, trimmed, _), _ = scc_case("cliques_%d" % k)
        count = 600 // k
        sizes = np.bincount(lab, minlength=N)
        assert comps == count + N - count * k and sorted(sizes[sizes > 1].tolist()) == [k] * count
        assert int(np.diff(cin.adj_indptr.astype(np.int64)).max()) == k and int(np.diff(cout.adj_indptr.astype(np.int64)).max()) == k
        lab, comps, passes, trimmed, _ = scc_case("dag_%d" % k)[3]
        assert np.array_equal(lab, np.arange(N)) and (comps, passes, trimmed) == (N, 0, N)
    cin, cout, _, (lab, comps, passes, trimmed, _), _ = scc_case("hub")
    assert comps == 1 + N - 601 and passes == 1 and np.bincount(lab).max() == 601
    assert int(np.diff(cin.adj_indptr.astype(np.int64)).max()) == 600 == int(np.diff(cout.adj_indptr.astype(np.int64)).max())
    cin, cout, _, (lab, comps, _, _, _), _ = scc_case("symmetric")
    assert cout is None and np.array_equal(lab, app._components_of(cin.adj_indptr, cin.adj_indices, cin.adj_data, N).astype(np.uint32))
    # the anchors of the random cases: components and passes, natural priorities and a seeded permutation
    for name, k in (("random_300_500", 164), ("random_300_1500", 3), ("random_1000_1400", 704)):
        n = scc_case(name)[0].num_rows
        for variant in (name, name + "_perm"):
            lab, comps, passes, _, _ = scc_case(variant)[3]
            assert comps - (n - int(name.split("_")[1])) == k and passes == 1, variant


def test_bowtie_labels_by_construction():
    s, d, used = _bowtie()
    where = np.random.default_rng(16).permutation(N)[:used]
    lab = scc_case("bowtie")[3][0]
    core = where[100:300]
    assert np.all(lab[core] == core.min()) and np.all(lab[where[440:442]] == where[440:442].min())
    rest = np.setdiff1d(np.arange(N), np.concatenate([core, where[440:442]]))
    assert np.array_equal(lab[rest], rest)                               # the trees, the tendrils and the unused vertices: singletons
    assert scc_case("bowtie")[3][1] == N - 200 - 2 + 2


def test_labels_do_not_depend_on_the_priorities_while_passes_may():
    for name in ("bowtie", "random_300_500", "random_1000_1400", "chain_asc"):
        cin, _, _, (lab, comps, passes, trimmed, _), (src, dst) = scc_case(name)
        n = cin.num_rows
        degrees = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
        for order in ("random", "largest_first"):
            got = scc_model(n, src, dst, io.coloring_priorities(degrees, order, 3))
            assert np.array_equal(got[0], lab) and got[1] == comps, (name, order)
    assert scc_case("chain_asc")[3][2] == 40 and scc_case("chain_asc_prio")[3][2] == 1


def test_validate_strong_components_accepts_the_truth_and_refuses_one_violation_per_rule():
    cin, _, _, (lab, comps, _, _, _), _ = scc_case("bowtie")
    assert app.validate_strong_components(cin, lab) == comps
    assert app.validate_strong_components(cin, np.concatenate([lab, np.arange(N, N + 128, dtype=np.uint32)])) == comps + 128
    with pytest.raises(ValueError, match="100 labels for a 640 x 640 matrix"):
        app.validate_strong_components(cin, lab[:100])
    big = np.flatnonzero(np.bincount(lab, minlength=N)[lab] == 200)        # the core
    root, other = int(big.min()), int(big.max())
    bad = lab.copy()
    bad[root] = other
    with pytest.raises(ValueError, match=r"vertex %d has label %d, which is above it \(rule 1\)" % (root, other)):
        app.validate_strong_components(cin, bad)
    second = int(np.sort(big)[1])
    bad = lab.copy()
    bad[big[big > second]] = second                                      # relabelled to a member that is not its own label's ...
    with pytest.raises(ValueError, match=r"whose own label is %d \(rule 1\)" % root):
        app.validate_strong_components(cin, bad)
    single = int(np.flatnonzero((lab == np.arange(N)) & (np.arange(N) > root) & (np.bincount(lab, minlength=N) == 1))[0])
    bad = lab.copy()
    bad[single] = root                                                   # a class that is not strongly connected
    with pytest.raises(ValueError, match=r"vertex %d (is not reached from|does not reach) its label %d inside its class \(rule 2\)" % (single, root)):
        app.validate_strong_components(cin, bad)
    # rule 3 alone: a two-cycle labelled as two singletons -- both classes are strongly connected, and they lie on a cycle
    two = _csr(128, [0, 1], [1, 0])
    assert app.validate_strong_components(two, np.r_[0, 0, np.arange(2, 128)]) == 127
    with pytest.raises(ValueError, match=r"the class of label 0 lies on a cycle of classes or behind one.*\(rule 3\)"):
        app.validate_strong_components(two, np.arange(128))


def _hand_made():
    """9 real vertices: the cycle 0 -> 1 -> 2 -> 0, the two-cycle 3 <-> 4, the singletons 5, 6 and 7, 8 unused, and between them
    2 -> 3, 1 -> 4 (a second edge between the same two components), 4 -> 5, 0 -> 5, 6 -> 0, 5 -> 7; a zero-valued entry 7 -> 6
    (no edge), a loop at 5 and a duplicate of 2 -> 3"""
    src = [0, 1, 2, 3, 4, 2, 1, 4, 0, 6, 5, 7, 5, 2]
    dst = [1, 2, 0, 4, 3, 3, 4, 5, 5, 0, 7, 6, 5, 3]
    data = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1]
    return _csr(9, dst, src, data)


def test_condensation_of_a_hand_made_graph():
    d = app.StronglyConnectedComponents(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        d.condensation()
    d.load_and_format_matrix(_hand_made())
    assert (d.n_, d.n_real_, d.graph_.nnz, d.symmetric_) == (128, 9, 11, False)
    # what run() leaves, from the model instead of the device
    src, dst = app._edges_of_pattern(d.graph_, 128)
    lab = scc_model(128, src, dst)[0]
    assert lab[:9].tolist() == [0, 0, 0, 3, 3, 5, 6, 7, 8]
    d.labels_ = lab
    d.component_labels_, sizes = np.unique(lab[:9], return_counts=True)
    d.num_components_ = 6
    dag, rank = d.condensation()
    assert rank.tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF, 1, 0xFFFFFFFF, 2, 3, 4, 5]
    assert (dag.num_rows, dag.num_cols, dag.nnz) == (6, 6, 5)
    rows = {v: dag.adj_indices[dag.adj_indptr[v]:dag.adj_indptr[v + 1]].tolist() for v in range(6)}
    # A[b, a]: a -> b.  {0,1,2} -> {3,4} once, {0,1,2} -> 5, {3,4} -> 5, 6 -> {0,1,2}, 5 -> 7
    assert rows == {0: [3], 1: [0], 2: [0, 1], 3: [], 4: [2], 5: []}
    assert app.validate_strong_components(dag, np.arange(6)) == 6          # a DAG: every vertex its own component


def test_driver_prepares_both_patterns_and_refuses_what_it_cannot_do(golden_dir):
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_scc reads the colour of every column"):
        app.StronglyConnectedComponents(comm=TwoRanks(), backend=CpuBackend())
    d = app.StronglyConnectedComponents(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (d.n_, d.n_real_) == (128, 8) and d.graph_.nnz == 7 and not d.symmetric_ and d.out_ is not None
    assert d.graph_out_.nnz == 7 and d.degrees_[:8].tolist() == [1, 2, 2, 2, 2, 2, 2, 1] and len(d.modules_) == 2
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    cin = scc_case("symmetric")[0]
    d.load_and_format_matrix(permute_rows(cin, 5))                        # the preparation sorts the rows
    assert d.symmetric_ and d.out_ is None and d.graph_out_ is None and len(d.modules_) == 1
    assert np.array_equal(d.graph_.adj_indices[:cin.nnz], cin.adj_indices) and d.n_ == N
    assert np.array_equal(d.degrees_, 2 * np.diff(cin.adj_indptr.astype(np.int64)))
    d.send_matrix_host_to_device()
    with pytest.raises(ValueError, match="order 'smallest_last' is none of natural, random, largest_first"):
        d.run(order="smallest_last")
    with pytest.raises(ValueError, match="priorities of shape"):
        d.run(priorities=np.zeros(7))


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("scc_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([SCC_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference


def test_walk_stars_the_last_entry_of_every_hub_row_decides():
    """the inputs of tests/test_gpu_walk.py::test_scc_*: without the last entry of the hub's long row (and its mirror in the other
    plan) the hub and its highest leaf are no component any more, in every variant -- a walk that skips that entry cannot give the
    expected labels; the loops change nothing the model sees; and the closed forms of the whole graph"""
    from test_gpu_walk import DEGREES, N as n, _stars, scc_stars, star_hubs
    hubs, last = star_hubs(1), _stars()[4]
    want = np.arange(n)
    want[last] = hubs
    for kind in ("in", "out"):
        for prio in (False, True):
            cin, cout, p, (lab, comps, passes, trimmed, _) = scc_stars(kind, False, prio)
            assert np.array_equal(lab, want) and (comps, passes, trimmed) == (n - 17, 1, 2519 - 17 + 24)
            assert np.array_equal(lab, scipy_labels(n, *app._edges_of_pattern(cin, n))[0])
            looped = scc_stars(kind, True, prio)
            assert looped[3][1:] == (comps, passes, trimmed, scc_stars(kind, False, prio)[3][4]) and np.array_equal(looped[3][0], lab)
            assert looped[0].nnz == cin.nnz + 2519 == looped[1].nnz
            long_rows = np.diff((looped[0] if kind == "in" else looped[1]).adj_indptr.astype(np.int64))[_stars()[3]]
            assert np.array_equal(long_rows, DEGREES)                      # (the loops are in the leaves' rows only)
            less = scc_stars(kind, False, prio, "last")[3]
            assert np.array_equal(less[0], np.arange(n)) and less[1:4] == (n, 0, n)
    cin, cout, p, (lab, comps, passes, trimmed, _) = scc_stars("sym", False, True)
    hub_of = _stars()[2]
    assert cout is None and np.array_equal(lab, np.where(hub_of >= 0, hub_of, np.arange(n))) and (comps, passes, trimmed) == (18 + 23, 1, 24)
    less = scc_stars("sym", False, True, "last")[3][0]
    assert np.all(less[last] == last) and np.all(lab[last] == hubs)
