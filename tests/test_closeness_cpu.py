"""CPU suite of the bit-parallel multi-source search and the closeness driver (gl_msbfs, SpMVPlan.msbfs, SpMVModule.msbfs,
app.ClosenessCentrality, app.validate_closeness): the export and its bindings exist; msbfs_model -- a numpy restatement of the
kernel, uint64 words, level by level, with the kernel's harmonic order -- equals one search per source and networkx's closeness,
harmonic centrality, eccentricity, diameter, radius, center and periphery; the validator accepts the model's output and refuses
every single corrupted word; the batching of the sources does not change the integers; the golden fixture is networkx's and the
model's.  tests/test_gpu_msbfs.py compares the kernels with msbfs_model and closeness_model (kept here).

far, reach, hops and the statistics are integers and harmonic is a fixed sequence of f64 operations, so the model is compared
exactly, harmonic as 64-bit words.  Only the comparison with networkx's floats is bounded:
  * closeness: networkx and closeness_of each make at most three roundings (reach / far, reach / (n - 1), their product) of
    positive numbers, each a relative error <= 2^-53, so the two values differ by at most 6 * 2^-53 (1 + 3 * 2^-53) relative:
    CLOSENESS_BOUND = 8 * 2^-53.
  * harmonic: every term is >= 0; the model makes one division and one addition per (batch, level), networkx one division and
    one addition per source, so the relative difference is at most 2 (batches * levels + sources) * 2^-53 to first order, and
    harmonic_bound doubles that for the higher orders."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from helpers import build_cpp_driver
from test_kcore_cpu import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSENESS_DRIVER = os.path.join(ROOT, "build", "closeness_driver")
HEADER = "graphlily_hip_msbfs.h"
DECL = ("int gl_msbfs(gl_spmv_plan plan, const uint32_t *h_sources, uint32_t k /* 1 .. 64 */, int accumulate, uint64_t *d_far, "
        "uint32_t *d_reach, double *d_harmonic, uint32_t *d_hops /* may be NULL: k * n words */, "
        "uint64_t *h_source_stats /* may be NULL: 3 * k HOST words */, uint64_t *h_stats /* may be NULL: 4 HOST words */);")
GOLDEN, EXPECTED = "closeness_whirl_csr_float32.npz", "closeness_whirl_expected.npz"
NONE = 0xFFFFFFFF
CLOSENESS_BOUND = 8.0 * 2.0 ** -53


def harmonic_bound(batches, levels, sources):
    return 4.0 * (batches * levels + sources) * 2.0 ** -53


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------ the host model
def msbfs_model(csr, sources, into=None, drop_last_entry_of=None):
    """gl_msbfs on the host, as the kernel does it: a uint64 word per vertex with bit j for sources[j], level by level
         next[v] = (OR over the u of row v of front[u]) & ~seen[v]
    over the rows of `csr` (row v: the predecessors of v; a column 0xffffffff or >= n is no edge), harmonic in the kernel's
    order.  `into` = (far, reach, harmonic) to accumulate into (copies are made).  -> (far uint64[n], reach uint32[n], harmonic
    float64[n], hops uint32[k, n], source_stats uint64[k, 3], (levels, full)).  drop_last_entry_of = v: row v without its last
    entry (what the early-exit tests need to know)."""
    n, k = csr.num_rows, len(sources)
    assert 1 <= k <= 64 and all(0 <= int(s) < n for s in sources)
    ip = csr.adj_indptr.astype(np.int64)[:n + 1].copy()
    idx = csr.adj_indices.astype(np.int64)[:ip[-1]]
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    keep = (idx < n) & (csr.adj_data[:ip[-1]] != 0)
    if drop_last_entry_of is not None:
        keep[ip[drop_last_entry_of + 1] - 1] = False
    row, idx = row[keep], idx[keep]
    mask = np.uint64((1 << k) - 1)
    seen = np.zeros(n, np.uint64)
    for j, s in enumerate(sources):
        seen[int(s)] |= np.uint64(1 << j)                             # 1 << j in Python integers: bit 63 included
    front = seen.copy()
    if into is None:
        far, reach, harmonic = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.float64)
    else:
        far, reach, harmonic = (np.array(x) for x in into)
    hops = np.full((k, n), NONE, np.uint32)
    for j, s in enumerate(sources):
        hops[j, int(s)] = 0
    stats = np.zeros((k, 3), np.uint64)
    d = 0
    while True:
        acc = np.zeros(n, np.uint64)
        np.bitwise_or.at(acc, row, front[idx])
        new = acc & ~seen
        if not new.any():
            break
        d += 1
        seen |= new
        c = np.zeros(n, np.int64)
        for j in range(k):
            got = (new >> np.uint64(j)) & np.uint64(1) != 0
            c += got
            hops[j, got] = d
            m = int(np.count_nonzero(got))
            if m:
                stats[j, 0] += np.uint64(m)
                stats[j, 1] += np.uint64(m * d)
                stats[j, 2] = np.uint64(d)
        hit = c > 0
        far[hit] += (c[hit] * d).astype(np.uint64)
        reach[hit] += c[hit].astype(np.uint32)
        harmonic[hit] = harmonic[hit] + c[hit].astype(np.float64) / np.float64(d)
        front = new
    return far, reach, harmonic, hops, stats, (d, int(np.count_nonzero(seen == mask)))


def closeness_model(csr, sources, batch=64):
    """the driver's batches through msbfs_model -> (far, reach, harmonic, hops uint32[len(sources), n], source_stats, levels)"""
    sources = [int(s) for s in sources]
    into, hops, stats, levels = None, [], [], 0
    for b in range(0, len(sources), batch):
        far, reach, harmonic, h, st, (lv, _) = msbfs_model(csr, sources[b:b + batch], into)
        into = (far, reach, harmonic)
        hops.append(h)
        stats.append(st)
        levels += lv
    return into[0], into[1], into[2], np.concatenate(hops), np.concatenate(stats), levels


def bfs_hops(csr, s):
    """one plain search from s over the rows of `csr` read as predecessor lists: a queue, one vertex at a time"""
    n = csr.num_rows
    succ = [[] for _ in range(n)]
    ip = csr.adj_indptr
    for v in range(n):
        for j in range(int(ip[v]), int(ip[v + 1])):
            u = int(csr.adj_indices[j])
            if u < n and csr.adj_data[j] != 0:
                succ[u].append(v)
    hops = np.full(n, NONE, np.uint32)
    hops[s] = 0
    queue = [s]
    for u in queue:
        for v in succ[u]:
            if hops[v] == NONE:
                hops[v] = hops[u] + 1
                queue.append(v)
    return hops


# ------------------------------------------------------------------ the named cases
def _edges(name):
    """-> (n, src, dst): the edges src[i] -> dst[i]"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "dipath_9":
        s = np.arange(8)
        return 9, s, s + 1
    if name == "cycle3_tail":                                        # 0 -> 1 -> 2 -> 0, 2 -> 3 -> 4; 5 isolated
        return 6, np.array([0, 1, 2, 2, 3]), np.array([1, 2, 0, 3, 4])
    if name == "random_directed_40":
        e = rng.integers(0, 40, (90, 2))
        e = np.unique(e[e[:, 0] != e[:, 1]], axis=0)
        return 40, e[:, 0], e[:, 1]
    if name == "random_undirected_48":                               # three components and two isolated vertices
        e = np.concatenate([rng.integers(0, 30, (50, 2)), rng.integers(30, 46, (24, 2))])
        e = e[e[:, 0] != e[:, 1]]
        return 48, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    if name == "grid_7x9":
        i, j = np.divmod(np.arange(63), 9)
        v = np.arange(63)
        a, b = np.concatenate([v[j < 8], v[i < 6]]), np.concatenate([v[j < 8] + 1, v[i < 6] + 9])
        return 63, np.concatenate([a, b]), np.concatenate([b, a])
    if name == "random_160":                                         # the batching graph: directed, 160 vertices
        e = rng.integers(0, 160, (420, 2))
        e = np.unique(e[e[:, 0] != e[:, 1]], axis=0)
        return 160, e[:, 0], e[:, 1]
    raise KeyError(name)


SMALL = ["dipath_9", "cycle3_tail", "random_directed_40", "random_undirected_48", "grid_7x9"]


@functools.lru_cache(maxsize=None)
def closeness_case(name):
    """-> (csr_in, csr_out or None): io.simple_pattern's matrices of the named graph (row v of csr_in: the predecessors of v);
    read-only, shared by both test files"""
    n, s, d = _edges(name)
    cin, cout, _ = io.simple_pattern(_csr(n, d, s))
    for m in (cin, cout):
        if m is not None:
            for arr in (m.adj_indptr, m.adj_indices, m.adj_data):
                arr.setflags(write=False)
    return cin, cout


def nx_graph(cin, directed):
    import networkx as nx
    G = nx.DiGraph() if directed else nx.Graph()
    G.add_nodes_from(range(cin.num_rows))
    dst = np.repeat(np.arange(cin.num_rows), np.diff(cin.adj_indptr.astype(np.int64)))
    G.add_edges_from(zip(cin.adj_indices.tolist(), dst.tolist()))
    return G


def hub_case(degree, k):
    """The early-exit inputs: vertex 0 is a hub whose row lists the vertices 1 .. degree; the sources 0 .. k - 2 are the
    vertices 1 .. k - 1 (among the hub's first eight entries), source k - 1 is the hub's LAST entry, vertex `degree`, and
    nothing else feeds the hub: only that last entry delivers bit k - 1.  -> (csr_in, sources)"""
    assert 2 <= k <= 9 and degree >= 9
    n = degree + 1 + 5
    cin = _csr(n, np.zeros(degree, np.int64), np.arange(1, degree + 1))
    return cin, list(range(1, k)) + [degree]


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_msbfs"), "libgraphlily_hip.so does not export gl_msbfs"
    assert len(L.gl_msbfs.argtypes) == 10
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_msbfs"]
    assert "gl_msbfs" not in capi.EXPORTS and "gl_msbfs" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.msbfs) and callable(M.SpMVModule.msbfs)
    assert callable(app.ClosenessCentrality.run) and callable(app.validate_closeness) and callable(app.closeness_of)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void msbfs(const uint32_t *sources, uint32_t k, bool accumulate, DeviceBuffer far, DeviceBuffer reach, DeviceBuffer harmonic" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    closeness_h = open(os.path.join(ROOT, "include", "graphlily", "app", "closeness.h")).read()
    for piece in ("class ClosenessCentrality : public app::PatternApp", "prepare(", "run(", "far()", "reach()", "harmonic()", "closeness()",
                  "hops()", "eccentricity()", "source_reach()", "source_far()", "diameter()", "radius()", "center()", "periphery()",
                  "batches()", "levels()", "launches()", "util_simple_pattern"):
        assert piece in closeness_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_msbfs.hip" in make and HEADER in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "closeness_driver.cpp" in entry
    plan_h = open(os.path.join(ROOT, "graphlily_amd", "csrc", "gl_spmv_plan.h")).read()
    assert "d_msbfs_scratch" in plan_h and "d_msbfs_scratch" in open(os.path.join(ROOT, "graphlily_amd", "csrc", "gl_spmv_plan.cpp")).read()


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_msbfs(None, None, 1, 0, None, None, None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


@pytest.mark.parametrize("name", SMALL + ["random_160"])
def test_model_equals_one_search_per_source(name):
    cin, cout = closeness_case(name)
    n = cin.num_rows
    sources = list(range(n))[::-1][:64]                               # descending: bit j is NOT vertex j
    far, reach, harmonic, hops, stats, (levels, full) = msbfs_model(cin, sources)
    want = np.stack([bfs_hops(cin, s) for s in sources])
    assert np.array_equal(hops, want)
    finite = np.where(want == NONE, 0, want).astype(np.int64)
    assert np.array_equal(far, finite.sum(axis=0).astype(np.uint64)) and np.array_equal(reach, np.count_nonzero(finite, axis=0))
    assert np.array_equal(stats[:, 0], np.count_nonzero(finite, axis=1)) and np.array_equal(stats[:, 1], finite.sum(axis=1))
    assert np.array_equal(stats[:, 2], finite.max(axis=1)) and levels == finite.max()
    assert full == np.count_nonzero(np.all(want != NONE, axis=0))
    h = np.zeros(n)
    for d in range(1, levels + 1):                                    # the same ordered loop, from the distance rows
        c = np.count_nonzero(want == d, axis=0)
        h[c > 0] = h[c > 0] + c[c > 0] / np.float64(d)
    assert np.array_equal(bits64(harmonic), bits64(h))
    sums = app._closeness_sums(want)                                  # the validator's own loop agrees
    assert np.array_equal(sums[0], far) and np.array_equal(sums[1], reach) and np.array_equal(bits64(sums[2]), bits64(harmonic))
    # the transposed pattern's rows measure the distances TO the sources
    if cout is not None:
        back = msbfs_model(cout, sources)[3]
        every = np.stack([bfs_hops(cin, s) for s in range(n)])
        assert np.array_equal(back, every[:, sources].T)


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_networkx(name):
    import networkx as nx
    cin, cout = closeness_case(name)
    n, directed = cin.num_rows, cout is not None
    G = nx_graph(cin, directed)
    every = list(range(n))
    for reverse in ((False, True) if directed else (False,)):
        H = G.reverse() if reverse else G
        far, reach, harmonic, hops, stats, levels = closeness_model(cout if reverse else cin, every)
        for wf in (True, False):
            want = nx.closeness_centrality(H, wf_improved=wf)
            got = app.closeness_of(far, reach, n, wf)
            ref = np.array([want[v] for v in every])
            assert np.array_equal(got == 0, ref == 0) and np.all(np.abs(got - ref) <= CLOSENESS_BOUND * ref), (name, reverse, wf)
        some = every[3::4]
        part = closeness_model(cout if reverse else cin, some)
        want = nx.harmonic_centrality(H, sources=some)
        ref = np.array([want[v] for v in every])
        bound = harmonic_bound(1, part[5], len(some))
        assert np.array_equal(part[2] == 0, ref == 0) and np.all(np.abs(part[2] - ref) <= bound * ref), (name, reverse)
        # distances FROM every vertex: networkx's eccentricity needs them all finite, so compare it per strongly connected piece
        ecc = stats[:, 2].astype(np.int64)
        lengths = dict(nx.all_pairs_shortest_path_length(H))
        assert ecc.tolist() == [max(lengths[v].values()) for v in every]
        assert np.array_equal(hops, np.array([[lengths[s].get(v, NONE) for v in every] for s in every], dtype=np.uint32))
        connected = nx.is_strongly_connected(H) if directed else nx.is_connected(H)
        if connected:
            who = np.arange(n)
            assert nx.eccentricity(H) == dict(zip(every, ecc.tolist()))
            assert nx.diameter(H) == ecc.max() and nx.radius(H) == ecc.min()
            assert sorted(nx.center(H)) == who[ecc == ecc.min()].tolist() and sorted(nx.periphery(H)) == who[ecc == ecc.max()].tolist()
    assert name != "grid_7x9" or connected                           # (at least this one reaches the eccentricity block)


def test_networkx_measures_incoming_distance_on_a_digraph():
    """the convention reverse=False follows: on 0 -> 1 -> 2 vertex 2 has the incoming distances 1 and 2, vertex 0 none"""
    import networkx as nx
    G = nx.DiGraph([(0, 1), (1, 2)])
    assert nx.closeness_centrality(G) == {0: 0.0, 1: 0.5, 2: 2.0 / 3.0}
    assert nx.harmonic_centrality(G) == {0: 0, 1: 1.0, 2: 1.5}
    cin = io.simple_pattern(_csr(3, [1, 2], [0, 1]))[0]
    far, reach, harmonic = closeness_model(cin, [0, 1, 2])[:3]
    assert far.tolist() == [0, 1, 3] and reach.tolist() == [0, 1, 2] and harmonic.tolist() == [0.0, 1.0, 1.5]
    assert app.closeness_of(far, reach, 3).tolist() == [0.0, 0.5, 2.0 / 3.0]


def test_closed_forms_of_the_model():
    n = 70
    s = np.arange(n - 1)
    path = io.symmetrize_simple(_csr(n, s + 1, s))[0]
    for k in (1, 2, 31, 32, 33, 63, 64):
        far, reach, harmonic, hops, stats, (levels, full) = msbfs_model(path, list(range(k)))
        assert np.array_equal(hops, np.abs(np.arange(n)[None, :] - np.arange(k)[:, None]))
        assert levels == n - 1 and full == n and np.array_equal(stats[:, 2], np.maximum(np.arange(k), n - 1 - np.arange(k)))
    far, reach, harmonic, hops, stats, (levels, full) = msbfs_model(path, [5, 5, 9])       # a source given twice counts twice
    assert far[5] == 4 and reach[5] == 1 and far[9] == 8 and reach[9] == 2 and np.array_equal(hops[0], hops[1]) and far[7] == 6
    empty = _csr(7, [], [])
    far, reach, harmonic, hops, stats, (levels, full) = msbfs_model(empty, [3, 4])
    assert not far.any() and not reach.any() and not harmonic.any() and levels == 0 and full == 0 and not stats.any()
    assert hops[0, 3] == 0 and hops[1, 4] == 0 and np.count_nonzero(hops == NONE) == 12
    assert msbfs_model(empty, [3])[5] == (0, 1) and msbfs_model(empty, [3, 3])[5] == (0, 1)
    zeros = _csr(4, [1, 2, 3], [0, 1, 2], [1.0, 0.0, 1.0])            # the stored zero is no edge
    assert msbfs_model(zeros, [0])[3][0].tolist() == [0, 1, NONE, NONE]


@pytest.mark.parametrize("degree", [9, 257])
@pytest.mark.parametrize("k", [3, 9])
def test_early_exit_inputs_depend_on_their_last_entry(degree, k):
    """what tests/test_gpu_msbfs.py's early-exit cases rely on: without the hub's last entry the hub never meets source k - 1"""
    cin, sources = hub_case(degree, k)
    full = msbfs_model(cin, sources)
    cut = msbfs_model(cin, sources, drop_last_entry_of=0)
    assert full[3][k - 1, 0] == 1 and cut[3][k - 1, 0] == NONE and full[1][0] == k and cut[1][0] == k - 1
    assert not np.array_equal(full[0], cut[0]) and not np.array_equal(bits64(full[2]), bits64(cut[2]))
    assert np.array_equal(full[3][:k - 1], cut[3][:k - 1])            # the first k - 1 bits arrive within the first eight entries
    assert all(s <= 8 for s in sources[:-1]) and sources[-1] == degree == cin.adj_indices[cin.adj_indptr[1] - 1]


@pytest.mark.parametrize("count", [65, 129])
def test_batching_of_the_sources_does_not_change_the_integers(count):
    cin, _ = closeness_case("random_160")
    rng = np.random.default_rng(count)
    sources = rng.permutation(160)[:count].tolist()
    far, reach, harmonic, hops, stats, _ = closeness_model(cin, sources)
    want = np.stack([bfs_hops(cin, s) for s in sources])
    assert np.array_equal(hops, want)
    for other in (sorted(sources), sources[::-1], rng.permutation(sources).tolist()):
        f2, r2, h2, hops2, stats2, _ = closeness_model(cin, other)
        assert np.array_equal(far, f2) and np.array_equal(reach, r2)
        assert np.array_equal(hops2, want[[sources.index(s) for s in other]])
        assert np.all(np.abs(h2 - harmonic) <= harmonic_bound(3, int(stats[:, 2].max()), 0) * harmonic)
    for batch in (1, 7, 32):                                          # ... nor does the batch size
        f2, r2 = closeness_model(cin, sources, batch)[:2]
        assert np.array_equal(far, f2) and np.array_equal(reach, r2)
    assert app.validate_closeness(cin, far, reach, harmonic, sources, hops=hops) == int(stats[:, 2].max())
    if count == 129:                                                  # the harmonic sum is a function of the SEQUENCE
        assert any(not np.array_equal(bits64(closeness_model(cin, o)[2]), bits64(harmonic)) for o in (sorted(sources), sources[::-1]))


@pytest.mark.parametrize("name", SMALL)
def test_validator_accepts_the_model_and_refuses_every_corrupted_word(name):
    cin, cout = closeness_case(name)
    n = cin.num_rows
    for reverse in (False, True):
        walk = cout if (reverse and cout is not None) else cin
        sources = list(range(n))[1::2]
        far, reach, harmonic, hops, stats, _ = closeness_model(walk, sources)
        diameter = int(stats[:, 2].max())
        assert app.validate_closeness(cin, far, reach, harmonic, sources, reverse=reverse, hops=hops) == diameter
        assert app.validate_closeness(cin, far, reach, sources=sources, reverse=reverse) == diameter
        padded = [np.concatenate([x, np.zeros(5, x.dtype)]) for x in (far, reach, harmonic)]
        assert app.validate_closeness(cin, *padded, sources, reverse=reverse) == diameter
        for v in range(n):
            for which, message in ((0, "vertex %d has far" % v), (1, "vertex %d has reach" % v), (2, "vertex %d has harmonic" % v)):
                arrays = [far.copy(), reach.copy(), harmonic.copy()]
                if which == 2:
                    arrays[2].view(np.uint64)[v] ^= np.uint64(1)      # one bit of the last place
                else:
                    arrays[which][v] += 1
                with pytest.raises(ValueError, match=message):
                    app.validate_closeness(cin, *arrays, sources, reverse=reverse)
        bad = hops.copy()
        bad[len(sources) // 2, n // 2] ^= 1
        with pytest.raises(ValueError, match=r"hops\[%d, %d\]" % (len(sources) // 2, n // 2)):
            app.validate_closeness(cin, far, reach, harmonic, sources, reverse=reverse, hops=bad)
    with pytest.raises(ValueError, match="given twice"):
        app.validate_closeness(cin, far, reach, sources=[0, 0])
    with pytest.raises(ValueError, match="a source outside"):
        app.validate_closeness(cin, far, reach, sources=[n])
    with pytest.raises(ValueError, match="values for a"):
        app.validate_closeness(cin, far[:-1], reach[:-1])


def test_validator_reads_the_graph_as_the_driver_does():
    """directed=False takes every edge in both directions; a stored zero, a loop and a duplicate are no edges"""
    raw = _csr(5, [1, 2, 2, 3, 3, 4], [0, 1, 1, 3, 2, 3], [1, 1, 1, 1, 1, 0])      # 0 -> 1 -> 2 (twice) -> 3 (a loop), 3 -> 4 stored as 0
    far, reach, harmonic = closeness_model(io.simple_pattern(raw)[0], range(5))[:3]
    assert far.tolist() == [0, 1, 3, 6, 0] and app.validate_closeness(raw, far, reach, harmonic) == 3
    sym = io.symmetrize_simple(raw)[0]
    f2, r2, h2 = closeness_model(sym, range(5))[:3]
    assert f2.tolist() == [6, 4, 4, 6, 0] and app.validate_closeness(raw, f2, r2, h2, directed=False) == 3
    with pytest.raises(ValueError, match="vertex 0 has far"):
        app.validate_closeness(raw, f2, r2, h2)


def _golden_model(golden_dir):
    raw = io.load_csr_matrix_from_float_npz(os.path.join(golden_dir, GOLDEN))
    cin, cout, sym = io.simple_pattern(raw)
    return raw, cin, cout


def test_golden_fixture_is_networkx_and_the_models(golden_dir):
    """tests/golden/closeness_whirl_csr_float32.npz: 44 vertices under a seeded permutation -- a directed cycle of 16 with six
    chords, three tails of 4 that leave it, two feeders of 3 that enter it, a separate directed triangle and seven isolated
    vertices --, one edge stored twice, a loop, a stored zero and rows stored unsorted.  The expected arrays were recorded from
    networkx (closeness with both wf values, harmonic centrality, in both directions) and from msbfs_model."""
    import networkx as nx
    raw, cin, cout = _golden_model(golden_dir)
    want = np.load(os.path.join(golden_dir, EXPECTED))
    n = 44
    assert (raw.num_rows, raw.num_cols) == (n, n) and cin.nnz == raw.nnz - 3 and cout is not None
    G = nx_graph(cin, True)
    for reverse, tag in ((False, "in"), (True, "out")):
        far, reach, harmonic, hops, stats, levels = closeness_model(cout if reverse else cin, range(n))
        assert np.array_equal(want["far_" + tag], far) and np.array_equal(want["reach_" + tag], reach)
        assert np.array_equal(want["harmonic_bits_" + tag], bits64(harmonic)) and np.array_equal(want["hops_" + tag], hops)
        assert np.array_equal(want["source_stats_" + tag], stats)
        H = G.reverse() if reverse else G
        for wf in (True, False):
            ref = nx.closeness_centrality(H, wf_improved=wf)
            ref = np.array([ref[v] for v in range(n)])
            assert np.array_equal(want["nx_closeness_%s_%d" % (tag, wf)], ref)
            got = app.closeness_of(far, reach, n, wf)
            assert np.array_equal(got == 0, ref == 0) and np.all(np.abs(got - ref) <= CLOSENESS_BOUND * ref)
        ref = want["nx_harmonic_" + tag]
        assert np.all(np.abs(harmonic - ref) <= harmonic_bound(1, levels, n) * ref) and np.array_equal(harmonic == 0, ref == 0)
        assert app.validate_closeness(raw, far, reach, harmonic, reverse=reverse, hops=hops) == int(stats[:, 2].max())
    assert int(want["source_stats_in"][:, 2].max()) >= 8               # deep enough to have several levels


def test_driver_prepares_both_patterns_and_refuses_what_it_cannot_do(golden_dir):
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_msbfs reads the frontier word of every column"):
        app.ClosenessCentrality(comm=TwoRanks(), backend=CpuBackend())
    d = app.ClosenessCentrality(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"))
    assert (d.n_, d.n_real_) == (128, 8) and d.graph_.nnz == 7 and d.directed_ and d.out_ is not None
    assert d.graph_out_.nnz == 7 and len(d.modules_) == 2
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, "line_8_csr_float32.npz"), directed=False)
    assert d.graph_.nnz == 14 and not d.directed_ and d.out_ is None and len(d.modules_) == 1
    raw, cin, cout = _golden_model(golden_dir)
    d.load_and_format_matrix(os.path.join(golden_dir, GOLDEN))
    assert (d.n_, d.n_real_, d.directed_) == (128, 44, True) and d.graph_.nnz == cin.nnz == d.graph_out_.nnz
    assert np.array_equal(d.graph_out_.adj_indices, cout.adj_indices) and len(d.modules_) == 2
    sym = closeness_case("grid_7x9")[0]
    d.load_and_format_matrix(sym.copy())                               # a CSRMatrix goes straight in
    assert not d.directed_ and d.out_ is None and len(d.modules_) == 1 and d.n_ == 128
    d.load_and_format_matrix(sym.copy(), directed=True)                # ... two plans on request
    assert d.directed_ and d.out_ is not None and len(d.modules_) == 2


def test_closeness_of_handles_the_edges():
    assert app.closeness_of([0, 2, 3], [0, 2, 1], 3).tolist() == [0.0, 1.0, (1.0 / 3.0) * 0.5]
    assert app.closeness_of([0, 2, 3], [0, 2, 1], 3, wf_improved=False).tolist() == [0.0, 1.0, 1.0 / 3.0]
    assert app.closeness_of([0], [0], 1).tolist() == [0.0]


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("closeness_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([CLOSENESS_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
