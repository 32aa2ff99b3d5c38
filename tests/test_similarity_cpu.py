"""CPU suite of the neighbourhood-similarity kernel's host side (gl_similarity, SpMVPlan.similarity, SpMVModule.similarity,
app.Similarity, app.validate_similarity): the export and its bindings exist; similarity_model -- Python sets and integer sums --
and the measure formulas, restated here as free functions on Python numbers, equal networkx's common_neighbors,
jaccard_coefficient, preferential_attachment, adamic_adar_index and resource_allocation_index; the validator accepts the model's
results and refuses a flipped count, a wrong score and a misaligned array; the choice of the fixed point; two_hop_pairs and top_k;
the golden fixture is the model's.  tests/test_gpu_sim.py compares the kernel with similarity_model (kept here).

common, jaccard and preferential_attachment are compared with networkx EXACTLY: the same integers, and for jaccard the same single
f64 division.  The two weighted measures are fixed point (shift = 62 - bit_length(max degree)): a term round(2^shift / x) is the
f64 quotient rounded to an integer -- off by at most 1/2 unit, 2^-(shift + 1) after scaling, and by one f64 rounding of the
quotient, 2^-53 relative --, the integer sum is exact, and the conversion of the sum to f64 is one more rounding; networkx adds
its c terms in f64, at most c - 1 roundings of partial sums that never exceed the result, each term with the roundings of its
own logarithm and division.  Together: |got - want| <= c 2^-(shift + 1) + (c + 1) 2^-52 want (weighted_bound), derived, not measured."""
import math
import os
import re

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from cpu_backend import CpuBackend
from test_kcore_cpu import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMILARITY_DRIVER = os.path.join(ROOT, "build", "similarity_driver")
HEADER = "graphlily_hip_sim.h"
DECL = ("int gl_similarity(gl_spmv_plan plan, const uint32_t *d_pairs /* 2 m words: u0 v0 u1 v1 ... */, uint64_t m, "
        "const uint64_t *d_vertex_weight /* may be NULL: n words */, uint32_t *d_common /* m words */, "
        "uint64_t *d_weighted /* may be NULL: m words */, uint64_t *h_stats /* may be NULL: 4 HOST words */);")
GOLDEN, EXPECTED = "similarity_caves_csr_float32.npz", "similarity_caves_expected.npz"
NONE = 0xFFFFFFFF
MEASURES = ("common", "jaccard", "overlap", "sorensen", "cosine", "preferential_attachment", "adamic_adar", "resource_allocation")


# ------------------------------------------------------------------ the host model and the formulas
def similarity_model(csr, pairs, vertex_weight=None):
    """gl_similarity on the host: Python sets and integer sums modulo 2^64 over the rows of `csr` (row x: N(x)) -> (common
    uint32[m], weighted uint64[m]); a pair with a vertex >= num_rows gives (0xffffffff, 0)."""
    n = csr.num_rows
    ip = csr.adj_indptr.astype(np.int64)
    rows = {}

    def row(x):
        if x not in rows:
            rows[x] = set(csr.adj_indices[ip[x]:ip[x + 1]].tolist())
        return rows[x]

    w = None if vertex_weight is None else [int(x) for x in np.asarray(vertex_weight).tolist()]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    common, weighted = np.zeros(pairs.shape[0], np.uint32), np.zeros(pairs.shape[0], np.uint64)
    for i, (u, v) in enumerate(pairs.tolist()):
        if u >= n or v >= n:
            common[i] = NONE
            continue
        both = row(u) & row(v)
        common[i] = len(both)
        if w is not None:
            weighted[i] = sum(w[x] for x in both) % (1 << 64)
    return common, weighted


def deferred_model(csr, pairs, cap):
    """-> the pairs in range whose shorter row has more than `cap` entries: the ones gl_similarity defers"""
    deg = np.diff(csr.adj_indptr.astype(np.int64))
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ok = (pairs < csr.num_rows).all(axis=1)
    return int(np.count_nonzero(np.minimum(deg[pairs[ok, 0]], deg[pairs[ok, 1]]) > cap))


def shift_of(max_degree):
    return 62 - int(max_degree).bit_length()


def tables_of(degrees):
    """-> (aa, ra, shift) as lists of Python ints: round-half-even of the f64 quotients 2^shift / ln(d) and 2^shift / d, d >= 2"""
    deg = [int(d) for d in np.asarray(degrees).tolist()]
    shift = shift_of(max(deg) if deg else 0)
    one = float(2 ** shift)
    return ([int(round(one / math.log(d))) if d >= 2 else 0 for d in deg], [int(round(one / d)) if d >= 2 else 0 for d in deg], shift)


def measure_of(name, c, du, dv, weighted=0, shift=0):
    """one measure of one pair from Python ints, 0.0 where a denominator is 0"""
    c, du, dv = int(c), int(du), int(dv)
    if name == "common":
        return c
    if name == "preferential_attachment":
        return du * dv
    if name in ("adamic_adar", "resource_allocation"):
        return float(int(weighted)) * 2.0 ** -shift
    num, den = {"jaccard": (c, du + dv - c), "overlap": (c, min(du, dv)), "sorensen": (2 * c, du + dv),
                "cosine": (c, math.sqrt(float(du) * float(dv)))}[name]
    return float(num) / float(den) if den > 0 else 0.0


def weighted_bound(c, shift, want):
    return c * 2.0 ** -(shift + 1) + (c + 1) * 2.0 ** -52 * want


def model_result(sym, degrees, pairs, measures=MEASURES):
    """what app.Similarity.run returns, from the model and the formulas above -> {measure: array}"""
    aa, ra, shift = tables_of(degrees)
    common, waa = similarity_model(sym, pairs, aa)
    _, wra = similarity_model(sym, pairs, ra)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = {}
    for name in measures:
        w = waa if name == "adamic_adar" else wra
        vals = [measure_of(name, common[i], degrees[u], degrees[v], w[i], shift) for i, (u, v) in enumerate(pairs.tolist())]
        out[name] = np.array(vals, dtype={"common": np.uint32, "preferential_attachment": np.uint64}.get(name, np.float64))
    return out


# ------------------------------------------------------------------ the graphs
def nx_case(name):
    import networkx as nx
    if name.startswith("gnp"):
        _, n, p = name.split("_")
        return nx.gnp_random_graph(int(n), float(p), seed=int(n))
    return {"path": lambda: nx.path_graph(9), "star": lambda: nx.star_graph(12), "empty": lambda: nx.empty_graph(7),
            "two_cliques": lambda: nx.barbell_graph(6, 0)}[name]()


def sym_of(G):
    """-> (symmetric CSRMatrix, degrees) of a networkx graph on the vertices 0 .. n - 1"""
    n = G.number_of_nodes()
    e = np.array(list(G.edges()), dtype=np.int64).reshape(-1, 2)
    return io.symmetrize_simple(_csr(n, e[:, 0], e[:, 1]))


def all_pairs(n):
    u, v = np.triu_indices(n, 1)
    return np.stack([u, v], axis=1).astype(np.int64)


CASES = ["gnp_60_0.15", "gnp_200_0.05", "gnp_40_0.6", "path", "star", "two_cliques", "empty"]


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_similarity"), "libgraphlily_hip.so does not export gl_similarity"
    assert len(L.gl_similarity.argtypes) == 7
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_similarity"]
    assert "gl_similarity" not in capi.EXPORTS and "gl_similarity" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.similarity) and callable(M.SpMVModule.similarity)
    assert callable(app.Similarity.run) and callable(app.Similarity.run_edges) and callable(app.validate_similarity)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void similarity(const uint32_t *pairs, uint64_t m, uint32_t *common, uint64_t *weighted = nullptr" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    sim_h = open(os.path.join(ROOT, "include", "graphlily", "app", "similarity.h")).read()
    for piece in ("class Similarity : public app::PatternApp", "prepare(", "run(", "run_edges(", "score(", "common()", "shift()",
                  "adamic_adar_sums()", "resource_allocation_sums()", "launches()", "util_symmetrize_simple"):
        assert piece in sim_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_sim.hip" in make and HEADER in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "similarity_driver.cpp" in entry
    plan_h = open(os.path.join(ROOT, "graphlily_amd", "csrc", "gl_spmv_plan.h")).read()
    assert "d_sim_scratch" in plan_h and "d_sim_scratch" in open(os.path.join(ROOT, "graphlily_amd", "csrc", "gl_spmv_plan.cpp")).read()


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_similarity(None, None, 0, None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


@pytest.mark.parametrize("name", CASES)
def test_model_and_formulas_equal_networkx(name):
    import networkx as nx
    G = nx_case(name)
    n = G.number_of_nodes()
    sym, deg = sym_of(G)
    assert [d for _, d in sorted(G.degree())] == deg.tolist()
    pairs = all_pairs(n)
    ebunch = [tuple(p) for p in pairs.tolist()]
    got = model_result(sym, deg, pairs)
    common = [len(list(nx.common_neighbors(G, u, v))) for u, v in ebunch]
    assert got["common"].tolist() == common
    assert got["jaccard"].tolist() == [p for _, _, p in nx.jaccard_coefficient(G, ebunch)]                 # exactly: one f64 division
    assert got["preferential_attachment"].tolist() == [p for _, _, p in nx.preferential_attachment(G, ebunch)]
    shift = shift_of(int(deg.max()) if n else 0)
    worst = 0.0
    for key, index in (("adamic_adar", nx.adamic_adar_index), ("resource_allocation", nx.resource_allocation_index)):
        want = np.array([p for _, _, p in index(G, ebunch)], dtype=np.float64)
        err = np.abs(got[key] - want)
        bound = np.array([weighted_bound(c, shift, w) for c, w in zip(common, want.tolist())])
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert np.all(err <= bound), (key, int(np.argmax(err - bound)), float(err.max()))
        assert np.array_equal(got[key] == 0, want == 0)
    print("%s: shift %d, worst weighted error %.3g" % (name, shift, worst))
    # the remaining coefficients against their definitions on networkx's sets
    for i in range(0, len(ebunch), 7):
        u, v = ebunch[i]
        a, b = set(G[u]), set(G[v])
        c = len(a & b)
        assert got["overlap"][i] == (c / min(len(a), len(b)) if min(len(a), len(b)) else 0.0)
        assert got["sorensen"][i] == (2 * c / (len(a) + len(b)) if len(a) + len(b) else 0.0)
        assert got["cosine"][i] == (c / math.sqrt(len(a) * len(b)) if len(a) * len(b) else 0.0)


@pytest.mark.parametrize("name", ["gnp_60_0.15", "star", "empty"])
def test_driver_formulas_equal_the_free_functions(name):
    """app.similarity_tables / similarity_measure (numpy, what the driver runs) against tables_of / measure_of (Python numbers)"""
    sym, deg = sym_of(nx_case(name))
    aa, ra, shift = app.similarity_tables(deg)
    waa, wra, wshift = tables_of(deg)
    assert shift == wshift == app.similarity_shift(int(deg.max()) if deg.size else 0)
    assert aa.dtype == ra.dtype == np.uint64 and aa.tolist() == waa and ra.tolist() == wra
    pairs = all_pairs(sym.num_rows)
    want = model_result(sym, deg, pairs)
    common, sums = similarity_model(sym, pairs, aa)
    for key in MEASURES:
        w = sums if key == "adamic_adar" else similarity_model(sym, pairs, ra)[1]
        got = app.similarity_measure(key, common, deg[pairs[:, 0]], deg[pairs[:, 1]], w, shift)
        assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), key
    with pytest.raises(ValueError, match="unknown measure"):
        app.similarity_measure("dice", common, deg[pairs[:, 0]], deg[pairs[:, 1]])


@pytest.mark.parametrize("max_degree,shift", [(0, 62), (1, 61), (2, 60), (3, 60), (4, 59), (7, 59), (8, 58), (2 ** 20 - 1, 42), (2 ** 20, 41),
                                              (2 ** 32 - 1, 30)])
def test_shift_keeps_every_sum_below_2_63(max_degree, shift):
    assert shift_of(max_degree) == app.similarity_shift(max_degree) == shift
    if max_degree >= 2:
        largest = int(round(2.0 ** shift / math.log(2)))            # the largest weight any vertex can have
        assert largest < 2 ** (shift + 1) and max_degree * largest < 2 ** 63


def test_validator_accepts_the_model_and_rejects_corruptions():
    G = nx_case("gnp_60_0.15")
    sym, deg = sym_of(G)
    raw = sym.copy()
    pairs = all_pairs(60)[::3]
    good = model_result(sym, deg, pairs)
    app.validate_similarity(raw, pairs, good)
    app.validate_similarity(raw, pairs[:0], {k: v[:0] for k, v in good.items()})
    i = int(np.flatnonzero(good["common"] > 0)[0])
    bad = dict(good, common=good["common"].copy())
    bad["common"][i] ^= 1
    with pytest.raises(ValueError, match=r"pair %d = \(%d, %d\) has common" % (i, pairs[i, 0], pairs[i, 1])):
        app.validate_similarity(raw, pairs, bad)
    for key in ("jaccard", "cosine", "adamic_adar", "resource_allocation"):
        bad = dict(good)
        bad[key] = good[key].copy()
        bad[key][i] = np.nextafter(bad[key][i], 2.0)                # one unit in the last place
        with pytest.raises(ValueError, match="has %s" % key):
            app.validate_similarity(raw, pairs, bad)
    with pytest.raises(ValueError, match="has preferential_attachment"):
        app.validate_similarity(raw, pairs, dict(good, preferential_attachment=good["preferential_attachment"] + np.uint64(1)))
    with pytest.raises(ValueError, match="jaccard has the shape"):
        app.validate_similarity(raw, pairs, dict(good, jaccard=good["jaccard"][:-1]))
    with pytest.raises(ValueError, match="has common"):               # misaligned: the right values, one place further
        app.validate_similarity(raw, pairs, dict(good, common=np.roll(good["common"], 1)))
    with pytest.raises(ValueError, match="unknown measure"):
        app.validate_similarity(raw, pairs, {"dice": good["common"]})
    with pytest.raises(ValueError, match="outside"):
        app.validate_similarity(raw, np.array([[0, 60]]), {"common": np.zeros(1, np.uint32)})
    with pytest.raises(ValueError, match=r"shape \[m, 2\]"):
        app.validate_similarity(raw, np.arange(6), {})
    # the validator reads the matrix as the driver does: direction, duplicates, the diagonal and zero values are ignored
    messy = _csr(5, [0, 0, 1, 2, 2, 3, 3], [1, 1, 2, 2, 0, 4, 0], data=[1, 1, 1, 1, 1, 0, 1])
    app.validate_similarity(messy, [[1, 3], [0, 2], [0, 4]], {"common": np.array([1, 1, 0], np.uint32)})


def _hand_made():
    """0 - {1, 2, 3}; 4 - {1, 2, 3}; 5 - {1, 2}; 6 - {1}; 7 - {3}; 8 - {3}; 9 alone: from 0, vertex 4 shares three neighbours, 5
    two, 6, 7 and 8 one each (7 and 8 tie in every measure)"""
    e = [(0, 1), (0, 2), (0, 3), (4, 1), (4, 2), (4, 3), (5, 1), (5, 2), (6, 1), (7, 3), (8, 3)]
    return _csr(10, [a for a, _ in e], [b for _, b in e])


def _driver(m):
    d = app.Similarity(backend=CpuBackend())
    d.load_and_format_matrix(m)
    return d


def test_two_hop_pairs_and_top_k_on_a_hand_made_graph(monkeypatch):
    d = _driver(_hand_made())
    assert (d.n_real_, d.graph_.nnz, d.shift_) == (10, 22, shift_of(4)) and d.degrees_[:10].tolist() == [3, 4, 3, 4, 3, 2, 1, 1, 1, 0]
    assert d.two_hop_pairs([0]).tolist() == [[0, 4], [0, 5], [0, 6], [0, 7], [0, 8]]
    assert d.two_hop_pairs([6, 0, 6]).tolist() == [[0, 4], [0, 5], [0, 6], [0, 7], [0, 8], [6, 0], [6, 4], [6, 5]]
    assert d.two_hop_pairs([9]).shape == (0, 2) and d.two_hop_pairs([]).shape == (0, 2)
    assert d.two_hop_pairs([1]).tolist() == [[1, 2], [1, 3]]           # through 0, 4 and 5: distinct pairs
    assert d.two_hop_pairs([0], limit=5).shape == (5, 2)
    with pytest.raises(ValueError, match="more than limit = 4"):
        d.two_hop_pairs([0], limit=4)
    with pytest.raises(ValueError, match="outside the real vertices"):
        d.two_hop_pairs([10])
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.top_k(0, 3)
    # the ordering of top_k, with the kernel replaced by the model
    d.sent_ = True
    monkeypatch.setattr(d, "run", lambda pairs, measures: model_result(d.graph_, d.degrees_, pairs, measures))
    v, s = d.top_k(0, 3, "common")
    assert v.tolist() == [4, 5, 6] and s.tolist() == [3, 2, 1]           # the tie 6 / 7 / 8 goes to the smallest vertex
    v, s = d.top_k(0, 10, "jaccard")
    assert v.tolist() == [4, 5, 6, 7, 8] and s.tolist() == [1.0, 2 / 3, 1 / 3, 1 / 3, 1 / 3]
    v, s = d.top_k(0, 2, "adamic_adar")
    assert v.tolist() == [4, 5] and abs(s[0] - (2 / math.log(4) + 1 / math.log(3))) < 1e-15
    assert d.top_k(9, 3)[0].shape == (0,) and d.top_k(0, 0)[0].shape == (0,)


def test_driver_errors_that_need_no_device():
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_similarity reads the rows of both vertices"):
        app.Similarity(comm=TwoRanks(), backend=CpuBackend())
    d = app.Similarity(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run([[0, 1]])
    d.load_and_format_matrix(_hand_made())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run([[0, 1]])
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run_edges()
    with pytest.raises(ValueError, match="unknown measure 'dice'"):
        d.run([[0, 1]], measures=("common", "dice"))
    with pytest.raises(ValueError, match="unknown measure"):
        d.top_k(0, 3, "dice")
    d.sent_ = True                                                     # (the checks below come before anything is enqueued)
    for bad in ([[0, 10]], [[-1, 2]], [[0, 127]]):                      # 127: a padding vertex
        with pytest.raises(ValueError, match="outside the real vertices 0 .. 9"):
            d.run(bad)
    with pytest.raises(ValueError, match=r"shape \[m, 2\]"):
        d.run([0, 1, 2])
    with pytest.raises(ValueError, match=r"shape \[m, 2\]"):
        d.run(np.zeros((2, 2)))
    assert d.n_ == 128 and d.aa_.shape == (128,) and not d.aa_[9:].any()
    got = d.run([[0, 4], [9, 9]], measures="preferential_attachment")  # no kernel
    assert got["preferential_attachment"].tolist() == [9, 0] and got["preferential_attachment"].dtype == np.uint64


def test_golden_fixture_is_the_models(golden_dir):
    """tests/golden/similarity_caves_csr_float32.npz: 48 vertices under a seeded permutation -- four cliques of 8 in a ring, a hub
    joined to 20 vertices, a few pendant vertices and six isolated ones --, stored with direction, duplicates, a loop and zero-valued
    entries; the expected file holds every pair u <= v of the first 24 vertices with the model's counts and fixed-point sums"""
    raw = io.load_csr_matrix_from_float_npz(os.path.join(golden_dir, GOLDEN))
    want = np.load(os.path.join(golden_dir, EXPECTED))
    sym, deg = io.symmetrize_simple(raw.copy())
    assert raw.num_rows == 48 and sym.nnz < raw.nnz + np.count_nonzero(raw.adj_data != 0) and int(deg.max()) >= 20
    aa, ra, shift = tables_of(deg)
    pairs = want["pairs"]
    assert int(want["shift"]) == shift and pairs.shape == (300, 2)
    common, waa = similarity_model(sym, pairs, aa)
    assert np.array_equal(want["common"], common) and np.array_equal(want["adamic_adar"], waa)
    assert np.array_equal(want["resource_allocation"], similarity_model(sym, pairs, ra)[1])
    assert want["adamic_adar"].dtype == np.uint64 and common.max() >= 7 and np.count_nonzero(common == 0) > 50
    res = model_result(sym, deg, pairs)
    app.validate_similarity(raw, pairs, res)
    d = _driver(os.path.join(golden_dir, GOLDEN))
    assert (d.n_, d.n_real_, d.shift_) == (128, 48, shift) and np.array_equal(d.degrees_[:48], deg) and d.aa_[:48].tolist() == aa
