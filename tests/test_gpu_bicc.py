"""GPU parity of the biconnected components (gl_bicc, SpMVPlan.bicc, SpMVModule.bicc, app.BiconnectedComponents,
graphlily::app::BiconnectedComponents) against the host model kept in tests/test_bicc_cpu.py (bicc_model_of, which that file checks
against networkx, scipy and the closed forms).  Every array of the kernel -- the four outputs and the six intermediate arrays of
d_tree -- is a function of the graph, so every comparison is exact, and a failure names the first array, in the order of the phases,
and the first index that differ.  Every test runs with the default dealing of the rows and with bicc_cut=0, every output buffer
starts as garbage with 64 guard words behind it, and every case is called twice on one plan.

gl_rows.h asks a new caller of the contract and of the walk to add itself to tests/test_gpu_rows.py and tests/test_gpu_walk.py;
this caller's contract and walk tests are here instead and import the shared inputs from those modules."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_bicc_cpu import (BICC_DRIVER, CASES, DEGREES, EXPECTED, GOLDEN, RESULTS, TREE, bicc_case, bicc_model_of,
                           build_cpp_driver)
from test_cc_cpu import permute_rows
from test_gpu_rows import _bool_plan, _graph
from test_gpu_walk import N as STAR_N, _stars
from test_kcore_cpu import _csr

pytestmark = pytest.mark.gpu

GARBAGE = 0xdeadbeef
GUARD = 64


@pytest.fixture(autouse=True, params=[None, 0], ids=["thread_per_short_row", "wavefront_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of the rows -- a thread reads the first bicc_cut entries of its row, the
    wavefront takes over what is left -- and with bicc_cut=0, which hands every row to the wavefront"""
    set_knob(monkeypatch, "bicc_cut", request.param)


def _bicc(plan, n, nnz):
    """-> ({name: array} of the four outputs, the tree split into its six arrays, stats); the buffers start out as garbage, and
    the guard behind each must stay garbage"""
    sizes = {"block": nnz, "vertex_blocks": n, "edge_component": n, "tree": 6 * n}
    bufs = {k: capi.DeviceBuffer.from_host(np.full(max(1, s) + GUARD, GARBAGE, np.uint32)) for k, s in sizes.items()}
    stats = plan.bicc(bufs["block"], bufs["vertex_blocks"], bufs["edge_component"], bufs["tree"])
    capi.sync()
    assert len(stats) == 6 and 0xdeadbeefdeadbeef not in stats
    got = {}
    for k, s in sizes.items():
        words = bufs[k].read(np.uint32, max(1, s) + GUARD)
        assert np.all(words[s:] == GARBAGE), "gl_bicc wrote behind the %d words of %s" % (s, k)
        got[k] = words[:s]
    for i, k in enumerate(TREE):
        got[k] = got["tree"][i * n:(i + 1) * n]
    del got["tree"]
    return got, stats


def _compare(got, model, what=""):
    """the arrays in the order of the phases: the first one that differs names the phase that went wrong"""
    for k in TREE + RESULTS:
        want = model[k].astype(np.uint32)
        if not np.array_equal(got[k], want):
            i = int(np.flatnonzero(got[k] != want)[0])
            raise AssertionError("%s%s differs first at index %d: the device has %d, the model %d (%d words differ)"
                                 % (what, k, i, got[k][i], want[i], np.count_nonzero(got[k] != want)))


def _stats_of(model):
    return (model["blocks"], model["articulation"], model["bridges"], model["depth"]), model["trees"]


def _check(sym, model, plan=None, what=""):
    """all ten arrays and the stats are the model's; twice on one plan"""
    plan = _bool_plan(sym) if plan is None else plan
    for _ in range(2):                                               # (the second time from the cached verdicts and scratch)
        got, stats = _bicc(plan, sym.num_rows, sym.nnz)
        _compare(got, model, what)
        assert (stats[:4], stats[5]) == _stats_of(model) and stats[4] >= 1
    return got, stats


@pytest.mark.parametrize("name", CASES)
def test_every_named_case(gpu, name):
    _check(*bicc_case(name), what=name + ": ")


@pytest.mark.parametrize("cut", [0, 4, 8, None])
def test_walk_stars(gpu, monkeypatch, cut):
    """the stars of tests/test_gpu_walk.py: every edge is a bridge and a block of its own, labelled with the smaller of its two
    entries, and the hubs of degree >= 2 are the articulation points; that the last entry of a hub row decides this is shown in
    tests/test_bicc_cpu.py"""
    N = STAR_N
    set_knob(monkeypatch, "bicc_cut", cut)
    sym, _, hub_of, hubs, last = _stars()
    got, stats = _check(sym, bicc_model_of(sym))
    rows, cols, mirror = app._mirror_entries(sym.adj_indptr, sym.adj_indices, N)
    assert np.array_equal(got["block"], np.minimum(np.arange(sym.nnz), mirror))
    assert np.array_equal(np.flatnonzero(got["vertex_blocks"] >= 2), hubs[np.asarray(DEGREES) >= 2])
    assert np.array_equal(got["edge_component"], np.arange(N)) and stats[:3] == (2519, 16, 2519) and stats[5] == 18 + 23


@pytest.mark.parametrize("name", ["union5", "path", "cactus", "random_1000_1400", "broom_264", "k65"])
def test_results_do_not_depend_on_the_knobs(gpu, monkeypatch, name):
    sym, model = bicc_case(name)
    plan = _bool_plan(sym)
    _, default = _check(sym, model, plan)
    set_knob(monkeypatch, "bicc_batch", 1)
    _, single = _check(sym, model, plan)
    set_knob(monkeypatch, "bicc_batch", 7)
    set_knob(monkeypatch, "bicc_grid", 1)
    _, narrow = _check(sym, model, plan)
    assert single[:4] == default[:4] == narrow[:4] and single[5] == default[5] == narrow[5]


def test_cc_labels_are_the_same_bits_before_and_after(gpu):
    """gl_cc.hip's union-find moved into a header that gl_bicc.hip shares, and gl_bicc uses the context's doubling words"""
    for name in ("random_1000_1400", "union5", "path"):
        sym, model = bicc_case(name)
        n = sym.num_rows
        plan = _bool_plan(sym)

        def labels():
            out = capi.DeviceBuffer.from_host(np.full(n + 1, GARBAGE, np.uint32))
            plan.cc_labels(out, capi.DeviceBuffer(4, ptr=out.ptr + 4 * n, keepalive=out))
            capi.sync()
            return out.read(np.uint32, n + 1)
        before = labels()
        _check(sym, model, plan)
        after = labels()
        assert np.array_equal(before, after) and before[n] == model["trees"] == app.validate_components(sym, before[:n])
        assert np.array_equal(np.flatnonzero(before[:n] == np.arange(n)), np.flatnonzero(model["level"] == 0))


def test_plan_without_entries_gives_the_trivial_answer(gpu):
    sym, model = bicc_case("empty")
    plan = capi.SpMVPlan(128, 128, sym.adj_indptr, sym.adj_indices, sym.adj_data, 0, 128, flags=capi.GL_PLAN_BOOLEAN)
    for _ in range(2):
        got, stats = _bicc(plan, 128, 0)
        _compare(got, model)
        assert stats[:4] == (0, 0, 0, 0) and stats[5] == 128 and 1 <= stats[4] <= 2
    block = capi.DeviceBuffer.from_host(np.full(16, GARBAGE, np.uint32))
    assert plan.bicc(block)[5] == 128 and np.all(block.read(np.uint32, 16) == GARBAGE)


def test_contract(gpu):
    """the refusals of kRowsSymmetric, in gl_truss' wording, leave the outputs and the plan untouched"""
    sym, model = bicc_case("random_300_1500")
    n, nnz = sym.num_rows, sym.nnz
    plan = _bool_plan(sym)

    def still_works():
        _compare(_bicc(plan, n, nnz)[0], model)
    still_works()
    out = capi.DeviceBuffer.from_host(np.full(nnz + 8 * n, GARBAGE, np.uint32))
    view = lambda first, count: capi.DeviceBuffer(4 * count, ptr=out.ptr + 4 * first, keepalive=out)       # noqa: E731
    vb, ec, tree = view(nnz, n), view(nnz + n, n), view(nnz + 2 * n, 6 * n)

    def refused(p, needle):
        for _ in range(2):                                           # (the second time from the cached verdict)
            with pytest.raises(capi.GraphLilyError) as e:
                p.bicc(out, vb, ec, tree)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
            assert "gl_bicc" in str(e.value)
        assert np.all(out.read(np.uint32, nnz + 8 * n) == GARBAGE), "a refused call writes nothing"
        still_works()
    general = capi.SpMVPlan(n, n, sym.adj_indptr, sym.adj_indices, sym.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "row copy")
    refused(_bool_plan(sym, 0, n // 2), "row shard")
    refused(_bool_plan(sym, n // 2, n), "row shard")
    sh = permute_rows(sym, 77)
    assert not np.array_equal(sh.adj_indices, sym.adj_indices)
    refused(_bool_plan(sh), "io.symmetrize_simple")                  # unsorted rows
    ip = sym.adj_indptr.astype(np.int64)
    v = int(np.flatnonzero(np.diff(ip) >= 2)[0])
    dup = sym.copy()
    dup.adj_indices = sym.adj_indices.copy()
    dup.adj_indices[ip[v] + 1] = dup.adj_indices[ip[v]]              # a duplicate column
    refused(_bool_plan(dup), "strictly ascending")
    z = sym.copy()
    z.adj_data = sym.adj_data.copy()
    z.adj_data[ip[v]] = 0.0                                          # a zero-valued entry: column 0xffffffff in the row copy
    refused(_bool_plan(z), "strictly ascending")
    wide = io.CSRMatrix(n, n + 128, sym.adj_data, sym.adj_indices, sym.adj_indptr)
    refused(_bool_plan(wide), "num_rows == num_cols")
    one_way = _csr(n, [0, 1, 1], [1, 0, 2])                          # (1, 2) without (2, 1)
    for needle in ("not symmetric", "io.symmetrize_simple"):
        refused(_bool_plan(one_way), needle)
    both = _graph(n, [0, 1], [1, 2])                                 # with the edge's other copy it is accepted
    got, stats = _bicc(_bool_plan(both), n, both.nnz)
    assert got["block"].tolist() == [0, 0, 2, 2] and stats[:4] == (2, 1, 2, 2) and stats[5] == n - 2
    with pytest.raises(capi.GraphLilyError) as e:
        plan.bicc(None)
    assert e.value.code == capi.GL_ERR_INVALID_ARG
    for args in ((out, out), (out, vb, vb), (out, vb, ec, ec), (out, None, None, out), (out, view(nnz - 1, n)),
                 (out, None, view(nnz + 2 * n + 5, n), tree)):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.bicc(*args)
        assert e.value.code == capi.GL_ERR_INVALID_ARG, args
    assert capi.lib().gl_bicc(None, ctypes.c_void_p(out.ptr), None, None, None, None) == capi.GL_ERR_INVALID_ARG
    assert np.all(out.read(np.uint32, nnz + 8 * n) == GARBAGE)
    # the optional outputs, one at a time
    for which in range(3):
        args = [None, None, None]
        args[which] = (vb, ec, tree)[which]
        plan.bicc(out, *args)
        capi.sync()
        words = out.read(np.uint32, nnz + 8 * n)
        assert np.array_equal(words[:nnz], model["block"].astype(np.uint32))
        want = np.full(8 * n, GARBAGE, np.uint32)
        if which == 0:
            want[:n] = model["vertex_blocks"]
        elif which == 1:
            want[n:2 * n] = model["edge_component"]
        else:
            want[2 * n:] = np.concatenate([model[k] for k in TREE])
        assert np.array_equal(words[nnz:], want), which
        out.write(np.full(nnz + 8 * n, GARBAGE, np.uint32))
    still_works()


def _module(m):
    mod = M.SpMVModule(M.num_hbm_channels, 1024, 256)
    mod.set_semiring(M.LogicalSemiring)
    mod.set_mask_type(M.kNoMask)
    mod.set_up_runtime()
    mod.load_and_format_matrix(m.copy(), True)
    mod.send_matrix_host_to_device()
    return mod


def test_module_layer(gpu):
    sym, model = bicc_case("cactus")
    n, nnz = sym.num_rows, sym.nnz
    mod = _module(sym)
    block, vb = (capi.DeviceBuffer.from_host(np.full(k, GARBAGE, np.uint32)) for k in (nnz, n))
    stats = mod.bicc(block, vb)
    capi.sync()
    assert np.array_equal(block.read(np.uint32, nnz), model["block"]) and np.array_equal(vb.read(np.uint32, n), model["vertex_blocks"])
    assert (stats[:4], stats[5]) == _stats_of(model)
    ec, tree = (capi.DeviceBuffer.from_host(np.full(k, GARBAGE, np.uint32)) for k in (n, 6 * n))
    assert mod.bicc(block, None, ec, tree)[:4] == stats[:4]
    capi.sync()
    assert np.array_equal(ec.read(np.uint32, n), model["edge_component"])
    assert np.array_equal(tree.read(np.uint32, 6 * n), np.concatenate([model[k] for k in TREE]))


def _driver(m):
    d = app.BiconnectedComponents(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True)
    d.send_matrix_host_to_device()
    return d


def test_driver_on_the_golden_cactus(gpu, golden_dir):
    """tests/golden/bicc_cactus_csr_float32.npz: 40 cycles of 3 .. 7 vertices in a chain, 161 vertices, every edge stored one way,
    the rows unsorted, with a loop, a duplicate and a zero-valued entry; bicc_cactus_expected.npz holds the model's answer"""
    path = os.path.join(golden_dir, GOLDEN)
    raw = io.load_csr_matrix_from_float_npz(path)
    expected = np.load(os.path.join(golden_dir, EXPECTED))
    assert (raw.num_rows, raw.num_cols) == (161, 161)
    d = _driver(path)
    n = d.n_
    assert (n, d.n_real_, d.graph_.nnz) == (256, 161, 400)
    model = bicc_model_of(d.graph_)
    for edge_components in (False, True):
        got = d.run(edge_components=edge_components)
        assert got.dtype == np.uint32 and got.shape == (400,) and d.block_ is got
        assert np.array_equal(got, expected["bicc_block"]) and np.array_equal(got, model["block"])
        assert np.array_equal(d.vertex_blocks_, model["vertex_blocks"]) and np.array_equal(d.vertex_blocks_[:161], expected["bicc_vertex_blocks"])
        assert np.array_equal(d.articulation_, model["vertex_blocks"] >= 2) and np.array_equal(d.bridge_, model["bridge"])
        assert (d.num_blocks_, d.num_articulation_, d.num_bridges_, d.num_trees_, d.depth_) == (40, 39, 0, 1, model["depth"])
        assert d.launches_ >= 3 * d.depth_ and not d.vertex_blocks_[161:].any()
        assert np.array_equal(d.block_labels_, np.unique(got)) and int(d.block_sizes_.sum()) == 200 and d.largest_block_ == 7
        assert np.array_equal(d.block_sizes_, np.bincount(got)[d.block_labels_] // 2)
        if edge_components:
            assert np.array_equal(d.edge_component_, model["edge_component"]) and not d.edge_component_[:161].any()
            assert np.array_equal(d.edge_component_[161:], np.arange(161, n))
        else:
            assert d.edge_component_ is None
    assert app.validate_biconnected(raw, got) == 40
    assert app.validate_biconnected(d.graph_, got, d.vertex_blocks_, d.edge_component_) == 40
    tree, block_rank, cut_rank = d.block_cut_tree()
    assert (tree.num_rows, tree.nnz) == (40 + 39, 2 * 78) and app.validate_components(tree, np.zeros(79, np.int64)) == 1
    assert np.array_equal(np.flatnonzero(block_rank != 0xFFFFFFFF), d.block_labels_)
    assert np.array_equal(np.flatnonzero(cut_rank != 0xFFFFFFFF), np.flatnonzero(d.articulation_))
    inner = np.diff(tree.adj_indptr.astype(np.int64))
    assert sorted(inner[:40].tolist()) == [1, 1] + [2] * 38 and np.all(inner[40:] == 2)       # a chain of blocks
    # a graph with bridges through the driver: a path with a triangle at its end
    d2 = _driver(_csr(8, [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 3]))
    d2.run(edge_components=True)
    assert (d2.num_blocks_, d2.num_articulation_, d2.num_bridges_, d2.num_trees_) == (4, 3, 3, 1 + 2)
    assert d2.edge_component_[:8].tolist() == [0, 1, 2, 3, 3, 3, 6, 7] and d2.largest_block_ == 3
    assert app.validate_biconnected(d2.graph_, d2.block_, d2.vertex_blocks_, d2.edge_component_) == 4
    d3 = _driver(_csr(8, [], []))                                    # ... and one without edges
    assert d3.run(edge_components=True).shape == (0,) and (d3.num_blocks_, d3.num_trees_, d3.largest_block_) == (0, 8, 0)
    assert np.array_equal(d3.edge_component_, np.arange(d3.n_)) and not d3.vertex_blocks_.any()


def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, golden_dir):
    build_cpp_driver("bicc_driver.cpp")
    path = os.path.join(golden_dir, GOLDEN)
    r = subprocess.run([BICC_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BiconnectedComponents::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(path)
    want = d.run(edge_components=True)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_block.bin"), dtype=np.uint32), want)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_vertex_blocks.bin"), dtype=np.uint32), d.vertex_blocks_)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_edge_component.bin"), dtype=np.uint32), d.edge_component_)
    checksum = 0
    for c in want.tolist():
        checksum = (checksum * 1000003 + c + 1) & 0xFFFFFFFFFFFFFFFF
    for line in ("blocks: %d" % d.num_blocks_, "articulation points: %d" % d.num_articulation_, "bridges: %d" % d.num_bridges_,
                 "trees: %d" % d.num_trees_, "depth: %d" % d.depth_, "checksum: %d" % checksum):
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])
