"""CPU suite of the biconnected components (gl_bicc, SpMVPlan.bicc, SpMVModule.bicc, app.BiconnectedComponents,
app.validate_biconnected): the export and its bindings exist; the host model of the kernel's rules -- Tarjan and Vishkin's algorithm
over the deterministic BFS forest, phase by phase as include/graphlily_hip_bicc.h states them -- equals networkx (articulation
points, bridges, blocks as edge sets) and scipy (the 2-edge-connected components) on every named case and meets the closed forms;
the depth-first search inside app.validate_biconnected equals the model; the validator accepts the truth and refuses one violation
per rule; the block-cut tree of a hand-made graph is the one worked out by hand; the driver prepares the symmetric matrix and
refuses what it cannot do; the C++ driver compiles against include/.  tests/test_gpu_bicc.py compares the kernels with bicc_model
(kept here) on the cases of bicc_case, array by array."""
import functools
import itertools
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
BICC_DRIVER = os.path.join(ROOT, "build", "bicc_driver")
HEADER = "graphlily_hip_bicc.h"
DECL = ("int gl_bicc(gl_spmv_plan plan, uint32_t *d_block /* nnz */, uint32_t *d_vertex_blocks /* num_rows, may be NULL */, "
        "uint32_t *d_edge_component /* num_rows, may be NULL */, uint32_t *d_tree /* 6 num_rows, may be NULL */, "
        "uint64_t *h_stats /* 6 HOST words, may be NULL */);")
GOLDEN = "bicc_cactus_csr_float32.npz"            # 40 cycles in a chain, stored one way, rows unsorted, a loop, a duplicate, a zero
EXPECTED = "bicc_cactus_expected.npz"             # ... and what the model gives on it: bicc_block, bicc_vertex_blocks
TREE = ("level", "parent", "pre", "nd", "low", "high")
RESULTS = ("block", "vertex_blocks", "edge_component")
# the hub degrees of tests/test_gpu_walk.py (DEGREES, asserted equal below): rows that end on every side of a four-entry step, of
# the cuts (8 and 32), of the wavefront (64) and of the 256-entry takeover step
DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257, 8 + 256, 8 + 257, 32 + 512, 32 + 513]


# ------------------------------------------------------------------ the host model
def _min_labels(n, x, y):
    """the classes of the pairs (x[i], y[i]) over n elements, each named by its smallest member"""
    order = np.argsort(x, kind="stable")
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(x, minlength=n), out=indptr[1:])
    return app._components_of(indptr, y[order], None, n)


def bicc_model_of(sym):
    """The phases of gl_bicc.hip on the symmetric simple matrix `sym` (rows ascending), in numpy -> a dict of level, parent, pre, nd,
    low, high (int64[n]), block (int64[nnz]), vertex_blocks, edge_component (int64[n]), bridge (bool[nnz]), depth, trees, blocks,
    articulation, bridges."""
    n, nnz = sym.num_rows, sym.nnz
    ip = sym.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    cols = sym.adj_indices.astype(np.int64)
    ident = np.arange(n, dtype=np.int64)
    # 1: the roots
    is_root = app._components_of(ip, cols, None, n) == ident
    # 2: the levels
    level = np.where(is_root, 0, -1).astype(np.int64)
    depth = 0
    while True:
        new = np.unique(cols[(level[rows] == depth) & (level[cols] < 0)])
        if new.size == 0:
            break
        depth += 1
        level[new] = depth
    assert np.all(level >= 0)
    # 3: the smallest neighbour one level up
    parent = np.full(n, n, np.int64)
    up = level[cols] == level[rows] - 1
    np.minimum.at(parent, rows[up], cols[up])
    parent[is_root] = ident[is_root]
    by_level = [np.flatnonzero(level == d) for d in range(depth + 1)]
    # 4: subtree sizes from the deepest level
    nd = np.ones(n, np.int64)
    for d in range(depth, 0, -1):
        np.add.at(nd, parent[by_level[d]], nd[by_level[d]])
    # 5: preorder from the top; the children of a row in entry order, which is ascending vertex order
    child_entry = (parent[cols] == rows) & (cols != rows)
    pre = np.zeros(n, np.int64)
    er, ec = rows[child_entry], cols[child_entry]
    before = np.cumsum(nd[ec]) - nd[ec]                                    # over ALL child entries, in entry order ...
    row_first = np.zeros(n, np.int64)
    if er.size:
        starts = np.flatnonzero(np.r_[True, er[1:] != er[:-1]])
        row_first[er[starts]] = before[starts]
    before -= row_first[er]                                                # ... made exclusive per row
    for d in range(depth):
        on = level[er] == d
        pre[ec[on]] = pre[er[on]] + 1 + before[on]
    # 6: low / high over the non-tree entries, then pushed up
    nontree = (parent[cols] != rows) & (parent[rows] != cols) & (cols != rows)
    low, high = pre.copy(), pre.copy()
    np.minimum.at(low, rows[nontree], pre[cols[nontree]])
    np.maximum.at(high, rows[nontree], pre[cols[nontree]])
    for d in range(depth, 0, -1):
        vs = by_level[d]
        np.minimum.at(low, parent[vs], low[vs])
        np.maximum.at(high, parent[vs], high[vs])
    # 7: the classes of the tree edges, each named by its child
    rule1 = child_entry & ~is_root[rows] & ((low[cols] < pre[rows]) | (high[cols] >= pre[rows] + nd[rows]))
    rule2 = nontree & (pre[rows] + nd[rows] <= pre[cols])
    pair = rule1 | rule2
    cls = _min_labels(n, rows[pair], cols[pair])
    # 8: the labels of the entries
    namer = np.where(child_entry, cols, np.where(parent[rows] == cols, rows, np.where(pre[cols] > pre[rows], cols, rows)))
    first = np.full(n, nnz, np.int64)
    np.minimum.at(first, cls[namer], np.arange(nnz, dtype=np.int64))
    block = first[cls[namer]]
    block[cols == rows] = 0xFFFFFFFF
    # 9: bridges, tops, vertex_blocks, the 2-edge-connected components
    flag = ~is_root & (low >= pre) & (high < pre + nd)
    bridge = (child_entry & flag[cols]) | ((parent[rows] == cols) & flag[rows] & (cols != rows))
    key = (level << 32) | ident
    top = np.full(n, 1 << 62, np.int64)
    np.minimum.at(top, cls[~is_root], key[~is_root])
    class_roots = np.flatnonzero(~is_root & (cls == ident))
    shallowest = top[class_roots] & 0xFFFFFFFF
    vertex_blocks = (~is_root).astype(np.int64) + np.bincount(parent[shallowest], minlength=n)
    keep = ~bridge & (cols != rows)
    edge_component = _min_labels(n, rows[keep], cols[keep])
    return dict(level=level, parent=parent, pre=pre, nd=nd, low=low, high=high, block=block, vertex_blocks=vertex_blocks,
                edge_component=edge_component, bridge=bridge, depth=depth, trees=int(is_root.sum()), blocks=int(class_roots.size),
                articulation=int(np.count_nonzero(vertex_blocks >= 2)), bridges=int(flag.sum()))


def bicc_model(n, a, b):
    """... on the undirected simple graph with the edges {a[i], b[i]} over n vertices -> (sym, the dict of bicc_model_of)"""
    sym = io.symmetrize_simple(_csr(n, a, b))[0]
    return sym, bicc_model_of(sym)


# ------------------------------------------------------------------ the named cases
def _pad(n):
    return (n + 127) // 128 * 128


def _clique(k, base=0):
    i, j = np.divmod(np.arange(k * k), k)
    return base + i[i < j], base + j[i < j]


def _cactus(cycles):
    """a chain of cycles of 3 .. 7 vertices, each sharing one vertex with the one before -> (a, b, vertices)"""
    a, b, at, free = [], [], 0, 1
    for i in range(cycles):
        ring = [at] + list(range(free, free + 2 + i % 5))
        free += 2 + i % 5
        a += ring
        b += ring[1:] + ring[:1]
        at = ring[len(ring) // 2]
    return np.array(a), np.array(b), free


def _broom(degree):
    """A hub of `degree` entries at level 1 of its tree: vertex 0 is the root and the hub's parent, vertex 1 the hub; the hub's other
    neighbours 2 .. degree are, in row order, children and -- every third of them, never the last -- neighbours of its own level
    (children of the root too, so the hub's row mixes its parent, non-tree entries and children).  Child number j carries a tail of
    j vertices, so that nd differs per child; the tails are numbered behind the row.  -> (a, b, vertices, the hub's last entry)"""
    if degree == 0:
        return np.array([0]), np.array([2]), 3, None                       # (the hub, vertex 1, is isolated)
    a, b, free, j = [0], [1], degree + 1, 0
    for i in range(degree - 1):
        u = 2 + i
        a.append(1), b.append(u)
        if i % 3 == 1 and i != degree - 2:
            a.append(0), b.append(u)
        else:
            chain = [u] + list(range(free, free + j))
            free += j
            a += chain[:-1]
            b += chain[1:]
            j += 1
    return np.array(a), np.array(b), free, (1, degree if degree > 1 else 0)


@functools.lru_cache(maxsize=None)
def _random_edges(n, m, seed):
    e = np.random.default_rng(seed).integers(0, n, (m, 2))
    return e[:, 0], e[:, 1]


@functools.lru_cache(maxsize=None)
def bicc_edges(name):
    """-> (n, a, b): the edges of a named case; n is a multiple of the drivers' padding"""
    kind, _, arg = name.partition("_")
    if name == "union5":                                                   # every graph on 5 labelled vertices, side by side
        pairs = list(itertools.combinations(range(5), 2))
        a = [5 * g + p[0] for g in range(1024) for i, p in enumerate(pairs) if g >> i & 1]
        b = [5 * g + p[1] for g in range(1024) for i, p in enumerate(pairs) if g >> i & 1]
        return 5120, np.array(a), np.array(b)
    if name == "path":
        return 3072, np.arange(2999), np.arange(1, 3000)
    if name == "cycle":
        return 2560, np.arange(2560), (np.arange(2560) + 1) % 2560
    if name == "barbell":
        (a1, b1), (a2, b2) = _clique(5), _clique(5, 5)
        return 128, np.concatenate([a1, a2, [4]]), np.concatenate([b1, b2, [5]])
    if name == "triangles":
        return 128, np.array([0, 1, 2, 2, 3, 4]), np.array([1, 2, 0, 3, 4, 2])
    if name == "star":
        return 128, np.zeros(100, np.int64), np.arange(1, 101)
    if name == "k65":
        return (128,) + _clique(65)
    if name == "grid":
        v = np.arange(640).reshape(20, 32)
        return 640, np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    if name == "cactus":
        a, b, used = _cactus(200)
        return _pad(used), a, b
    if name == "empty":
        return 128, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "random":
        n, m = (int(x) for x in arg.split("_")[:2])
        a, b = _random_edges(n, m, 7)
        if name.endswith("_perm"):
            where = np.random.default_rng(8).permutation(_pad(n))
            a, b = where[a], where[b]
        return _pad(n), a, b
    if kind == "broom":
        a, b, used, _ = _broom(int(arg))
        return _pad(used), a, b
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def bicc_case(name):
    """-> (sym, model): the symmetric matrix as io.symmetrize_simple prepares it and the dict of bicc_model_of; read-only arrays,
    shared by both test files"""
    n, a, b = bicc_edges(name)
    sym, model = bicc_model(n, a, b)
    for arr in (sym.adj_indptr, sym.adj_indices, sym.adj_data) + tuple(v for v in model.values() if isinstance(v, np.ndarray)):
        arr.setflags(write=False)
    return sym, model


BROOMS = ["broom_%d" % d for d in DEGREES]
CASES = (["union5", "path", "cycle", "barbell", "triangles", "star", "k65", "grid", "cactus", "random_1000_1400", "random_300_1500",
          "random_1000_1400_perm", "random_300_1500_perm"] + BROOMS)


def _networkx_truth(sym):
    """-> (block label per entry, articulation points, bridges as a set of (lo, hi), edge_component) from networkx and scipy"""
    import networkx as nx
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = sym.num_rows
    rows, cols, mirror = app._mirror_entries(sym.adj_indptr, sym.adj_indices, n)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(rows[rows < cols].tolist(), cols[rows < cols].tolist()))
    entry_of = {(int(r), int(c)): j for j, (r, c) in enumerate(zip(rows, cols))}
    block = np.full(sym.nnz, -1, np.int64)
    for edges in nx.biconnected_component_edges(G):
        members = np.array([entry_of[(u, v)] for u, v in edges] + [entry_of[(v, u)] for u, v in edges])
        block[members] = members.min()
    bridges = {(min(u, v), max(u, v)) for u, v in nx.bridges(G)}
    keep = np.array([(min(r, c), max(r, c)) not in bridges for r, c in zip(rows.tolist(), cols.tolist())], bool)
    k, comp = connected_components(sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n)), directed=False)
    smallest = np.full(k, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return block, set(nx.articulation_points(G)), bridges, smallest[comp]


# ------------------------------------------------------------------ the tests
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_bicc"), "libgraphlily_hip.so does not export gl_bicc"
    assert len(L.gl_bicc.argtypes) == 6
    text, names = _declared(HEADER)
    assert DECL in open(os.path.join(ROOT, "include", HEADER)).read() and '#include "graphlily_hip.h"' in text and 'extern "C"' in text
    assert sorted(capi.EXT_HEADERS[HEADER]) == names == ["gl_bicc"]
    assert all(hasattr(L, s) for s in capi.EXT_HEADERS[HEADER])
    assert "gl_bicc" not in capi.EXPORTS and "gl_bicc" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.bicc) and callable(M.SpMVModule.bicc)
    assert callable(app.BiconnectedComponents.run) and callable(app.BiconnectedComponents.block_cut_tree)
    assert callable(app.validate_biconnected)
    spmv_h = open(os.path.join(ROOT, "include", "graphlily", "module", "spmv_module.h")).read()
    assert "void bicc(DeviceBuffer block, DeviceBuffer vertex_blocks, DeviceBuffer edge_component, uint64_t *stats = nullptr)" in spmv_h
    assert '#include "%s"' % HEADER in spmv_h
    bicc_h = open(os.path.join(ROOT, "include", "graphlily", "app", "bicc.h")).read()
    for piece in ("class BiconnectedComponents : public app::PatternApp", "prepare(", "run(bool edge_components", "blocks()", "vertex_blocks()",
                  "edge_components()", "num_blocks()", "num_articulation_points()", "num_bridges()", "depth()", "launches()",
                  "util_symmetrize_simple"):
        assert piece in bicc_h
    make = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_bicc.hip" in make and HEADER in make and "gl_unionfind.h" in make
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "EXT_HEADERS" in entry and "bicc_driver.cpp" in entry


def test_entry_point_fails_loudly_without_a_gpu():
    if capi.device_count() == 0:
        assert capi.lib().gl_bicc(None, None, None, None, None, None) == capi.GL_ERR_NOT_INITIALIZED


@pytest.mark.parametrize("name", CASES + ["empty"])
def test_model_equals_networkx_and_scipy_on_every_case(name):
    sym, m = bicc_case(name)
    n = sym.num_rows
    block, cut, bridges, edge_component = _networkx_truth(sym)
    assert np.array_equal(m["block"], block)
    assert set(np.flatnonzero(m["vertex_blocks"] >= 2).tolist()) == cut and m["articulation"] == len(cut)
    rows, cols, _ = app._mirror_entries(sym.adj_indptr, sym.adj_indices, n)
    on = m["bridge"] & (rows < cols)
    assert set(zip(rows[on].tolist(), cols[on].tolist())) == bridges and m["bridges"] == len(bridges)
    assert np.array_equal(m["edge_component"], edge_component)
    assert m["blocks"] == np.unique(block).size
    # the blocks a vertex belongs to, and a bridge is a block of one edge
    distinct = np.bincount(np.unique(rows * max(sym.nnz, 1) + block) // max(sym.nnz, 1), minlength=n)
    assert np.array_equal(m["vertex_blocks"], distinct)
    assert np.array_equal(m["bridge"], np.bincount(block, minlength=max(sym.nnz, 1))[block] == 2)


@pytest.mark.parametrize("name", CASES + ["empty"])
def test_depth_first_search_of_the_validator_equals_the_model(name):
    sym, m = bicc_case(name)
    assert np.array_equal(app._blocks_of(sym.adj_indptr, sym.adj_indices, sym.num_rows), m["block"])
    assert app.validate_biconnected(sym, m["block"], m["vertex_blocks"], m["edge_component"]) == m["blocks"]


def test_closed_forms_of_the_model():
    sym, m = bicc_case("path")
    assert (m["blocks"], m["bridges"], m["articulation"], m["depth"], m["trees"]) == (2999, 2999, 2998, 2999, 1 + 72)
    assert m["bridge"].all() and np.array_equal(np.flatnonzero(m["vertex_blocks"] >= 2), np.arange(1, 2999))
    assert np.array_equal(m["edge_component"], np.arange(3072)) and np.array_equal(m["pre"][:3000], np.arange(3000))
    sym, m = bicc_case("cycle")
    assert (m["blocks"], m["bridges"], m["articulation"], m["depth"], m["trees"]) == (1, 0, 0, 1280, 1)
    assert np.all(m["block"] == 0) and np.all(m["vertex_blocks"] == 1) and np.all(m["edge_component"] == 0)
    sym, m = bicc_case("triangles")
    assert (m["blocks"], m["bridges"], m["articulation"]) == (2, 0, 1) and m["vertex_blocks"][:5].tolist() == [1, 1, 2, 1, 1]
    assert np.all(m["edge_component"][:5] == 0)
    sym, m = bicc_case("barbell")
    assert (m["blocks"], m["bridges"], m["articulation"]) == (3, 1, 2) and np.flatnonzero(m["vertex_blocks"] >= 2).tolist() == [4, 5]
    assert m["edge_component"][:10].tolist() == [0] * 5 + [5] * 5 and sorted(np.bincount(m["block"])[np.unique(m["block"])].tolist()) == [2, 20, 20]
    sym, m = bicc_case("star")
    assert (m["blocks"], m["bridges"], m["articulation"], m["depth"]) == (100, 100, 1, 1) and m["vertex_blocks"][0] == 100
    sym, m = bicc_case("k65")
    assert (m["blocks"], m["bridges"], m["articulation"], m["depth"], m["trees"]) == (1, 0, 0, 1, 1 + 63)
    assert np.all(m["block"] == 0) and m["nd"][0] == 65
    sym, m = bicc_case("grid")
    assert (m["blocks"], m["bridges"], m["articulation"], m["depth"], m["trees"]) == (1, 0, 0, 19 + 31, 1)
    sym, m = bicc_case("empty")
    assert (m["blocks"], m["bridges"], m["articulation"], m["depth"], m["trees"]) == (0, 0, 0, 0, 128) and m["block"].size == 0
    assert np.all(m["vertex_blocks"] == 0) and np.array_equal(m["edge_component"], np.arange(128)) and np.all(m["nd"] == 1)
    sym, m = bicc_case("cactus")
    assert (m["blocks"], m["bridges"], m["articulation"]) == (200, 0, 199)
    sym, m = bicc_case("union5")
    assert m["depth"] == 4 and m["trees"] == int((m["parent"] == np.arange(5120)).sum()) and m["blocks"] == np.unique(m["block"]).size


def test_brooms_are_what_the_gpu_suite_needs():
    """the hub is at level 1, its row has the degree asked for and mixes its parent, neighbours of its own level and children, the
    last entry is a child, and the children's subtrees all differ in size"""
    from test_gpu_walk import DEGREES as walk_degrees
    assert walk_degrees == DEGREES
    for d in DEGREES[1:]:
        sym, m = bicc_case("broom_%d" % d)
        ip = sym.adj_indptr.astype(np.int64)
        row = sym.adj_indices[ip[1]:ip[2]].astype(np.int64)
        assert row.size == d and m["level"][1] == 1 and m["parent"][1] == 0 and row[0] == 0
        kids = row[m["parent"][row] == 1]
        assert kids.size == (d - 1) - sum(1 for i in range(d - 1) if i % 3 == 1 and i != d - 2)
        if d > 1:
            assert row[-1] == kids[-1] and np.array_equal(m["nd"][kids], 1 + np.arange(kids.size))
            assert np.array_equal(m["pre"][kids], m["pre"][1] + 1 + np.cumsum(np.r_[0, m["nd"][kids][:-1]]))
        same = row[(m["level"][row] == 1)]
        assert same.size == d - 1 - kids.size and (d < 4 or same.size > 0)


def test_the_last_entry_of_every_hub_row_decides():
    """the walk inputs of tests/test_gpu_bicc.py, run through the model again without the last entry of every hub row (and its
    mirror): the answer changes, so a walk that skips that entry cannot give the expected arrays"""
    from test_gpu_walk import N as n, _star_edges, _stars
    sym, _, hub_of, hubs, last = _stars()
    m = bicc_model_of(sym)
    hub, leaf, kept = _star_edges("last")
    assert m["bridge"].all() and m["bridges"] == 2519 == m["blocks"]
    assert np.array_equal(np.flatnonzero(m["vertex_blocks"] >= 2), hubs[np.asarray(DEGREES) >= 2])
    less = bicc_model(n, hub[kept], leaf[kept])[1]
    assert less["blocks"] == 2519 - 17 and np.all(less["vertex_blocks"][last] == 0) and np.all(m["vertex_blocks"][last] == 1)
    assert np.array_equal(less["vertex_blocks"][hubs], m["vertex_blocks"][hubs] - (np.asarray(DEGREES) > 0))
    for d in DEGREES[2:]:
        nn, a, b = bicc_edges("broom_%d" % d)
        full = bicc_case("broom_%d" % d)[1]
        drop = ~((a == 1) & (b == d))
        assert np.count_nonzero(~drop) == 1
        cut = bicc_model(nn, a[drop], b[drop])[1]
        assert cut["trees"] == full["trees"] + 1 and cut["blocks"] == full["blocks"] - 1
        assert cut["nd"][1] < full["nd"][1] and cut["vertex_blocks"][1] == full["vertex_blocks"][1] - 1


def test_validate_biconnected_accepts_the_truth_and_refuses_one_violation_per_rule():
    sym, m = bicc_case("barbell")
    block, vb, ec = m["block"], m["vertex_blocks"], m["edge_component"]
    assert app.validate_biconnected(sym, block, vb, ec) == 3 and app.validate_biconnected(sym, block) == 3
    assert app.validate_biconnected(sym, block, np.r_[vb, np.zeros(128, np.int64)], np.r_[ec, np.arange(128, 256)]) == 3
    with pytest.raises(ValueError, match="7 labels for the 42 entries"):
        app.validate_biconnected(sym, block[:7])
    rows, cols, mirror = app._mirror_entries(sym.adj_indptr, sym.adj_indices, 128)
    bridge = int(np.flatnonzero(m["bridge"])[0])
    bad = block.copy()
    bad[bridge] = 0
    with pytest.raises(ValueError, match=r"entry %d \(4, 5\) is given block 0, its mirror entry %d block %d \(rule 1\)" % (bridge, mirror[bridge], block[bridge])):
        app.validate_biconnected(sym, bad)
    bad = block.copy()
    bad[block == 0] = mirror[0]                                          # a class named by an entry that is not its smallest
    with pytest.raises(ValueError, match=r"entry 0 has label %d, which is no entry at or below it \(rule 2\)" % mirror[0]):
        app.validate_biconnected(sym, bad)
    bad = block.copy()
    bad[m["bridge"]] = 0                                                 # the bridge put into the first clique's block
    with pytest.raises(ValueError, match=r"entry %d \(4, 5\) is given block 0, a depth-first search finds .* %d \(rule 3\)" % (bridge, block[bridge])):
        app.validate_biconnected(sym, bad)
    bad = vb.copy()
    bad[4] = 1
    with pytest.raises(ValueError, match=r"vertex 4 lies in 2 blocks, vertex_blocks says 1 \(rule 4\)"):
        app.validate_biconnected(sym, block, bad)
    with pytest.raises(ValueError, match=r"edge_component, on the graph without its bridges: .*\(rule 5\)"):
        app.validate_biconnected(sym, block, vb, np.r_[np.zeros(10, np.int64), np.arange(10, 128)])


def _hand_made():
    """8 real vertices: the triangle 0 1 2, the bridge 2 - 3, the square 3 4 5 6, the pendant 6 - 7; a loop at 4, a duplicate of
    (0, 1) and a zero-valued entry (7, 0), which is no edge"""
    a = [0, 1, 2, 2, 3, 4, 5, 6, 6, 4, 0, 7]
    b = [1, 2, 0, 3, 4, 5, 6, 3, 7, 4, 1, 0]
    d = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    return _csr(8, a, b, d)


def test_block_cut_tree_of_a_hand_made_graph():
    d = app.BiconnectedComponents(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        d.block_cut_tree()
    d.load_and_format_matrix(_hand_made())
    assert (d.n_, d.n_real_, d.graph_.nnz) == (128, 8, 18)
    m = bicc_model_of(d.graph_)                                          # what run() leaves, from the model instead of the device
    assert (m["blocks"], m["bridges"], m["articulation"], m["trees"]) == (4, 2, 3, 1 + 120)
    d.block_ = m["block"].astype(np.uint32)
    d.vertex_blocks_ = m["vertex_blocks"].astype(np.uint32)
    d.articulation_ = d.vertex_blocks_ >= 2
    d.block_labels_ = np.unique(d.block_)
    d.num_blocks_ = 4
    assert np.flatnonzero(d.articulation_).tolist() == [2, 3, 6] and m["edge_component"][:8].tolist() == [0, 0, 0, 3, 3, 3, 3, 7]
    tree, block_rank, cut_rank = d.block_cut_tree()
    assert (tree.num_rows, tree.num_cols, tree.nnz) == (7, 7, 12) and cut_rank[[2, 3, 6]].tolist() == [4, 5, 6]
    assert np.count_nonzero(cut_rank != 0xFFFFFFFF) == 3 and np.count_nonzero(block_rank != 0xFFFFFFFF) == 4
    # blocks by ascending label: the triangle (entry 0), the bridge 2 - 3, the square, the pendant 6 - 7
    ip = d.graph_.adj_indptr.astype(np.int64)
    tri, bridge, square, pendant = (int(block_rank[d.block_[ip[v]]]) for v in (0, 3, 4, 7))
    assert (tri, bridge, square, pendant) == (0, 1, 2, 3)
    rows = {v: tree.adj_indices[tree.adj_indptr[v]:tree.adj_indptr[v + 1]].tolist() for v in range(7)}
    assert rows == {0: [4], 1: [4, 5], 2: [5, 6], 3: [6], 4: [0, 1], 5: [1, 2], 6: [2, 3]}
    assert app.validate_components(tree, np.zeros(7, np.int64)) == 1     # a tree: connected, 7 nodes and 6 edges


def test_driver_prepares_the_matrix_and_refuses_what_it_cannot_do(golden_dir):
    class TwoRanks:
        rank, world_size, distributed = 0, 2, True
    with pytest.raises(NotImplementedError, match="row shards are not supported -- gl_bicc reads the level, the parent and the preorder"):
        app.BiconnectedComponents(comm=TwoRanks(), backend=CpuBackend())
    d = app.BiconnectedComponents(backend=CpuBackend())
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    d.load_and_format_matrix(os.path.join(golden_dir, GOLDEN))
    a, b, used = _cactus(40)
    want = io.symmetrize_simple(_csr(_pad(used), a, b))[0]
    assert (d.n_, d.n_real_) == (want.num_rows, used) and d.graph_.nnz == want.nnz == 2 * a.size
    assert np.array_equal(d.graph_.adj_indices, want.adj_indices) and np.array_equal(d.graph_.adj_indptr, want.adj_indptr)
    assert np.array_equal(d.degrees_, np.diff(want.adj_indptr.astype(np.int64)))
    with pytest.raises(RuntimeError, match="send_matrix_host_to_device"):
        d.run()
    golden = np.load(os.path.join(golden_dir, EXPECTED))
    m = bicc_model_of(d.graph_)
    assert np.array_equal(golden["bicc_block"], m["block"]) and np.array_equal(golden["bicc_vertex_blocks"], m["vertex_blocks"][:used])
    sym = bicc_case("random_300_1500")[0]
    d.load_and_format_matrix(permute_rows(sym, 5))                        # the preparation sorts the rows
    assert np.array_equal(d.graph_.adj_indices, sym.adj_indices) and d.n_ == sym.num_rows


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("bicc_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([BICC_DRIVER, str(tmp_path / "none.npz"), str(tmp_path)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
