"""GPU parity of the bit-parallel multi-source search (gl_msbfs, SpMVPlan.msbfs, SpMVModule.msbfs, app.ClosenessCentrality,
graphlily::app::ClosenessCentrality) against the host model kept in tests/test_closeness_cpu.py (msbfs_model, which that file
checks against one search per source and against networkx).  far, reach, hops and the statistics are integers and harmonic is a
fixed sequence of f64 operations, so every comparison is np.array_equal, harmonic as 64-bit words.  Every test runs with the
default dealing of the rows and with msbfs_cut=0; every output buffer starts as garbage with guard words behind it.  This caller's
contract and walk cases (gl_rows.h) live here."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_closeness_cpu import (CLOSENESS_DRIVER, GOLDEN, NONE, bits64, build_cpp_driver, closeness_case, closeness_model, hub_case,
                                msbfs_model, nx_graph)
from test_gpu_walk import CUTS, DEGREES, N as STAR_N, _stars
from test_kcore_cpu import _csr

pytestmark = pytest.mark.gpu

G32, G64 = 0xdeadbeef, 0xdeadbeefdeadbeef
GUARD = 64


@pytest.fixture(autouse=True, params=[None, 0], ids=["thread_per_short_row", "wavefront_per_row"])
def dealing(request, monkeypatch):
    """every test runs twice: with the default dealing of the rows -- a thread reads the first msbfs_cut entries of its rows,
    the wavefront takes over what is left -- and with msbfs_cut=0, which hands every row to the wavefront"""
    set_knob(monkeypatch, "msbfs_cut", request.param)


def _bool_plan(m, r0=0, r1=None):
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, m.num_rows if r1 is None else r1,
                         flags=capi.GL_PLAN_BOOLEAN)
    assert plan.info()["layout"] == "boolean" or m.nnz == 0
    return plan


class Out:
    """the four output arrays on the device: garbage (or `into`, to accumulate into) with GUARD guard words behind each"""

    def __init__(self, n, k, into=None, hops=True):
        self.n, self.k = n, k
        far = np.full(n + GUARD, G64, np.uint64)
        reach = np.full(n + GUARD, G32, np.uint32)
        harmonic = np.full(n + GUARD, G64, np.uint64)
        if into is not None:
            far[:n], reach[:n], harmonic[:n] = into[0], into[1], bits64(into[2])
        self.far, self.reach, self.harmonic = (capi.DeviceBuffer.from_host(x) for x in (far, reach, harmonic))
        self.hops = capi.DeviceBuffer.from_host(np.full(k * n + GUARD, G32, np.uint32)) if hops else None

    def read(self):
        """-> (far, reach, harmonic bits, hops or None); the guard words must still be garbage"""
        n, k = self.n, self.k
        far, reach, harmonic = self.far.read(np.uint64, n + GUARD), self.reach.read(np.uint32, n + GUARD), self.harmonic.read(np.uint64, n + GUARD)
        assert np.all(far[n:] == G64) and np.all(reach[n:] == G32) and np.all(harmonic[n:] == G64), "a guard word was written"
        hops = None
        if self.hops is not None:
            hops = self.hops.read(np.uint32, k * n + GUARD)
            assert np.all(hops[k * n:] == G32), "a guard word behind hops was written"
            hops = hops[:k * n].reshape(k, n)
        return far[:n], reach[:n], harmonic[:n], hops


def _msbfs(plan, n, sources, into=None, hops=True):
    """-> (far, reach, harmonic bits, hops, source_stats, stats)"""
    out = Out(n, len(sources), into, hops)
    source_stats, stats = plan.msbfs(sources, out.far, out.reach, out.harmonic, into is not None, out.hops)
    capi.sync()
    assert source_stats.shape == (len(sources), 3) and G64 not in source_stats and len(stats) == 4 and G64 not in stats and stats[3] == 0
    return out.read() + (source_stats, stats)


def _compare(got, want, what=""):
    far, reach, harmonic, hops, source_stats, stats = got
    wfar, wreach, wharmonic, whops, wstats, (levels, full) = want
    for name, a, b in (("far", far, wfar), ("reach", reach, wreach), ("harmonic", harmonic, bits64(wharmonic))):
        assert np.array_equal(a, b), "%s %s: first difference at vertex %d" % (what, name, int(np.flatnonzero(a != b)[0]))
    if hops is not None:
        assert np.array_equal(hops, whops), "%s hops: first difference at %s" % (what, [int(x[0]) for x in np.nonzero(hops != whops)])
    assert np.array_equal(source_stats, wstats), what
    assert stats[:2] == (levels, full) and stats[2] >= 1, (what, stats, levels, full)


def _check(csr, sources, plan=None, calls=2, what=""):
    plan = _bool_plan(csr) if plan is None else plan
    want = msbfs_model(csr, sources)
    for _ in range(calls):                                            # (the second time from the cached scratch: identical bits)
        got = _msbfs(plan, csr.num_rows, sources)
        _compare(got, want, what)
    return got


def _sym_path(k, n):
    s = np.arange(k - 1)
    return io.symmetrize_simple(_csr(n, s + 1, s))[0]


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 63, 64])
def test_every_bit_has_its_own_source(gpu, k):
    """a path of 70 vertices with source j at vertex j: hops is the closed form |v - j|, which a 32-bit shift, a swapped bit or a
    lost bit 63 breaks -- the sums alone would not show these, they are symmetric in the sources"""
    path = _sym_path(70, 70)
    got = _check(path, list(range(k)))
    assert np.array_equal(got[3], np.abs(np.arange(70)[None, :] - np.arange(k)[:, None]))
    assert got[5][0] == 69 and got[5][1] == 70
    got = _check(path, list(range(k))[::-1])                           # ... and bit j at vertex k - 1 - j
    assert np.array_equal(got[3], np.abs(np.arange(70)[None, :] - np.arange(k)[::-1, None]))


# ------------------------------------------------------------------ the driver's batches
def _driver(m, directed=None):
    d = app.ClosenessCentrality(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(m, True, directed)
    d.send_matrix_host_to_device()
    return d


def _driver_equals_model(d, sources, reverse=False, hops=True):
    walk = d.graph_out_ if reverse and d.graph_out_ is not None else d.graph_
    every = list(range(d.n_real_)) if sources is None else list(sources)
    far, reach, harmonic, whops, wstats, levels = closeness_model(walk, every)
    got = d.run(sources, reverse=reverse, hops=hops)
    assert got.dtype == np.float64 and got.shape == (d.n_,) and got is d.closeness_
    assert np.array_equal(d.far_, far) and np.array_equal(d.reach_, reach) and np.array_equal(bits64(d.harmonic_), bits64(harmonic))
    assert d.far_.dtype == np.uint64 and d.reach_.dtype == np.uint32 and d.harmonic_.dtype == np.float64
    assert d.sources_ == every and d.batches_ == (len(every) + 63) // 64 and d.levels_ == levels and d.launches_ >= d.batches_
    assert np.array_equal(d.source_reach_, wstats[:, 0]) and np.array_equal(d.source_far_, wstats[:, 1]) and np.array_equal(d.eccentricity_, wstats[:, 2])
    ecc = wstats[:, 2].astype(np.int64)
    assert d.diameter_ == ecc.max() and d.radius_ == ecc.min()
    assert np.array_equal(d.center_, np.asarray(every)[ecc == ecc.min()]) and np.array_equal(d.periphery_, np.asarray(every)[ecc == ecc.max()])
    if hops:
        assert d.hops_.dtype == np.uint32 and np.array_equal(d.hops_, whops)
    else:
        assert d.hops_ is None
    assert np.array_equal(bits64(got), bits64(app.closeness_of(far, reach, d.n_real_, True)))
    assert not d.far_[d.n_real_:].any() and not got[d.n_real_:].any()                   # the padding: isolated, never a source
    # the identities between the per-vertex and the per-source sums
    assert int(d.far_.sum()) == int(d.source_far_.sum()) and int(d.reach_.sum()) == int(d.source_reach_.sum())
    return got


@pytest.mark.parametrize("count", [65, 128, 129])
def test_driver_batches_equal_the_model(gpu, count):
    cin = closeness_case("random_160")[0]
    d = _driver(cin.copy())
    assert d.n_ == 256 and d.n_real_ == 160 and d.directed_
    sources = np.random.default_rng(count).permutation(160)[:count].tolist()
    _driver_equals_model(d, sources)
    _driver_equals_model(d, sources, reverse=True, hops=False)
    assert app.validate_closeness(cin, d.far_, d.reach_, d.harmonic_, sources, reverse=True) == d.diameter_
    with pytest.raises(ValueError, match="given twice"):
        d.run([3, 4, 3])
    with pytest.raises(ValueError, match="outside the real vertices"):
        d.run([160])


# ------------------------------------------------------------------ early exit with k < 64
def test_early_exit_on_a_complete_graph(gpu):
    i, j = np.divmod(np.arange(25), 5)
    k5 = _csr(5, i[i != j], j[i != j])
    got = _check(k5, [4, 0, 2])
    assert got[0].tolist() == [2, 3, 2, 3, 2] and got[5][:2] == (1, 5)


@pytest.mark.parametrize("degree", [9, 257])
@pytest.mark.parametrize("k", [3, 9])
def test_early_exit_needs_the_last_entry(gpu, degree, k):
    """the hub's first eight entries deliver k - 1 bits, its LAST entry alone the k-th (tests/test_closeness_cpu.py proves that
    the answer changes without that entry): a body that stops at the low k - 1 bits, or at a mask of ~0, shows here"""
    cin, sources = hub_case(degree, k)
    got = _check(cin, sources)
    assert got[3][k - 1, 0] == 1 and got[1][0] == k and got[5][1] == 1


# ------------------------------------------------------------------ the walk's boundaries
@pytest.mark.parametrize("cut", CUTS)
def test_walk_boundaries_on_the_star_union(gpu, monkeypatch, cut):
    """tests/test_gpu_walk.py's stars: hub degrees on every side of 4, 8, 32, 64, 256 and cut + 256; the sources are the HIGHEST
    leaf of every star, so the last entry of each hub row decides the hub's hops"""
    set_knob(monkeypatch, "msbfs_cut", cut)
    sym, _, hub_of, hubs, last = _stars()
    assert len(last) == 17 and sym.num_rows == STAR_N
    got = _check(sym, last.tolist())
    live = np.asarray(DEGREES) > 0
    assert np.array_equal(got[3][np.arange(17), hubs[live]], np.ones(17))
    assert np.array_equal(got[1][hubs[live]], np.ones(17)) and got[5][0] == 2


# ------------------------------------------------------------------ depth and gating
def test_results_do_not_depend_on_the_batch(gpu, monkeypatch):
    """a path of 300 vertices next to 20 isolated ones: 299 levels, more than one batch"""
    path = _sym_path(300, 320)
    plan = _bool_plan(path)
    sources = [0, 299, 150, 7, 310]
    want = msbfs_model(path, sources)
    assert want[5] == (299, 0)
    default = 16
    for batch in (1, 2, 7, None):
        set_knob(monkeypatch, "msbfs_batch", batch)
        got = _msbfs(plan, 320, sources)
        _compare(got, want, "batch %s" % batch)
        b = default if batch is None else batch
        assert got[5][0] == 299 and got[5][2] == 1 + b * ((300 + b - 1) // b), (batch, got[5])
    set_knob(monkeypatch, "msbfs_batch", 7)
    set_knob(monkeypatch, "msbfs_grid", 1)
    _compare(_msbfs(plan, 320, sources), want, "grid 1")


# ------------------------------------------------------------------ direction
@pytest.mark.parametrize("name", ["dipath_9", "cycle3_tail"])
def test_direction_on_the_plans(gpu, name):
    cin, cout = closeness_case(name)
    n = cin.num_rows
    sources = list(range(n))
    fwd, back = _check(cin, sources), _check(cout, sources)
    assert np.array_equal(fwd[3], back[3].T)                           # d(s, v) from one plan is d(v, s) from the other
    assert np.any(fwd[3] == NONE) and np.array_equal(fwd[0], np.where(fwd[3] == NONE, 0, fwd[3]).sum(axis=0))      # unreached: 0xffffffff, adds 0
    if name == "dipath_9":
        assert fwd[0].tolist() == [v * (v + 1) // 2 for v in range(9)] and back[0].tolist() == [v * (v + 1) // 2 for v in range(9)][::-1]


@pytest.mark.parametrize("reverse", [False, True])
def test_driver_on_the_golden_file(gpu, golden_dir, reverse):
    import networkx as nx
    path = os.path.join(golden_dir, GOLDEN)
    raw = io.load_csr_matrix_from_float_npz(path)
    d = _driver(path)
    assert (d.n_, d.n_real_, d.directed_) == (128, 44, True) and d.out_ is not None
    got = _driver_equals_model(d, None, reverse)
    want = np.load(os.path.join(golden_dir, "closeness_whirl_expected.npz"))
    tag = "out" if reverse else "in"
    assert np.array_equal(d.far_[:44], want["far_" + tag]) and np.array_equal(d.hops_[:, :44], want["hops_" + tag])
    assert np.array_equal(bits64(d.harmonic_[:44]), want["harmonic_bits_" + tag]) and np.all(d.hops_[:, 44:] == NONE)
    ref = want["nx_closeness_%s_1" % tag]
    assert np.array_equal(got[:44] == 0, ref == 0) and np.all(np.abs(got[:44] - ref) <= 8.0 * 2.0 ** -53 * ref)
    assert app.validate_closeness(raw, d.far_, d.reach_, d.harmonic_, reverse=reverse, hops=d.hops_) == d.diameter_
    flat = d.run(reverse=reverse, wf_improved=False)
    assert np.array_equal(bits64(flat), bits64(app.closeness_of(d.far_, d.reach_, 44, False))) and d.hops_ is None
    few = [5, 40, 17]
    _driver_equals_model(d, few, reverse)
    assert app.validate_closeness(raw, d.far_, d.reach_, d.harmonic_, few, reverse=reverse, hops=d.hops_) == d.diameter_


def test_diameter_is_networkx_on_a_connected_graph(gpu):
    import networkx as nx
    cin = closeness_case("grid_7x9")[0]
    d = _driver(cin.copy())
    assert not d.directed_ and d.out_ is None
    _driver_equals_model(d, None)
    G = nx_graph(cin, False)
    assert d.diameter_ == nx.diameter(G) == 14 and d.radius_ == nx.radius(G)
    assert sorted(d.center_.tolist()) == sorted(nx.center(G)) and sorted(d.periphery_.tolist()) == sorted(nx.periphery(G))
    assert np.array_equal(bits64(d.run(reverse=True)), bits64(d.closeness_))           # undirected: one plan, both directions
    e = _driver(cin.copy(), directed=True)                             # ... and as two plans
    _driver_equals_model(e, None, reverse=True)
    assert np.array_equal(e.far_, d.far_)


# ------------------------------------------------------------------ the contract
def test_refusals_and_invalid_arguments(gpu):
    cin = closeness_case("random_directed_40")[0]
    n = cin.num_rows
    plan = _bool_plan(cin)
    sources = [3, 9, 27]
    want = msbfs_model(cin, sources)
    out = Out(n, 3)

    def untouched():
        far, reach, harmonic, hops = out.read()
        assert np.all(far == G64) and np.all(reach == G32) and np.all(harmonic == G64) and np.all(hops == G32), "a refused call writes nothing"
        _compare(_msbfs(plan, n, sources), want)

    def refused(p, needle):
        for _ in range(2):
            with pytest.raises(capi.GraphLilyError) as e:
                p.msbfs(sources, out.far, out.reach, out.harmonic, False, out.hops)
            assert e.value.code == capi.GL_ERR_UNSUPPORTED and needle in str(e.value) and "gl_msbfs" in str(e.value), str(e.value)
        untouched()

    general = capi.SpMVPlan(n, n, cin.adj_indptr, cin.adj_indices, cin.adj_data)
    assert general.info()["layout"] != "boolean"
    refused(general, "the plan keeps no row copy")
    refused(_bool_plan(cin, 0, n // 2), "row shard")
    refused(_bool_plan(io.CSRMatrix(n, n + 128, cin.adj_data, cin.adj_indices, cin.adj_indptr)), "num_rows == num_cols")

    def invalid(needle, src, *bufs):
        with pytest.raises(capi.GraphLilyError) as e:
            plan.msbfs(src, *bufs)
        assert e.value.code == capi.GL_ERR_INVALID_ARG and needle in str(e.value), (needle, str(e.value))

    invalid("d_far != nullptr", sources, None, out.reach, out.harmonic)
    invalid("d_reach != nullptr", sources, out.far, None, out.harmonic)
    invalid("d_harmonic != nullptr", sources, out.far, out.reach, None)
    invalid("k >= 1u && k <= 64u", [], out.far, out.reach, out.harmonic)
    invalid("k >= 1u && k <= 64u", list(range(30)) + list(range(35)), out.far, out.reach, out.harmonic)
    invalid("source 2 is vertex 40 of 40", [3, 9, n], out.far, out.reach, out.harmonic)
    invalid("source 0 is vertex 4294967295", [0xFFFFFFFF], out.far, out.reach, out.harmonic)
    invalid("two output arrays overlap", sources, out.far, out.reach, out.far)
    invalid("two output arrays overlap", sources, out.far, out.reach, out.harmonic, False, out.reach)
    inside = capi.DeviceBuffer(4 * n, ptr=out.hops.ptr + 4 * 2 * n, keepalive=out.hops)       # the last of the three rows of hops
    invalid("two output arrays overlap", sources, out.far, inside, out.harmonic, False, out.hops)
    with pytest.raises(capi.GraphLilyError) as e:
        capi.check(capi.lib().gl_msbfs(None, None, 1, 0, None, None, None, None, None, None))
    assert e.value.code == capi.GL_ERR_INVALID_ARG and "plan != nullptr && h_sources != nullptr" in str(e.value)
    untouched()
    _compare(_msbfs(plan, n, sources, hops=False), want)             # d_hops may be NULL


def test_zero_valued_entries_are_no_edges(gpu):
    rng = np.random.default_rng(11)
    cin = closeness_case("random_160")[0]
    z = cin.copy()
    z.adj_data = cin.adj_data.copy()
    z.adj_data[rng.random(cin.nnz) < 0.3] = 0.0                        # stored as column 0xffffffff in the row copy
    assert 0 < np.count_nonzero(z.adj_data == 0) < z.nnz
    sources = rng.permutation(160)[:40].tolist()
    got = _check(z, sources)
    assert not np.array_equal(got[0], msbfs_model(cin, sources)[0])
    sh = cin.copy()                                                    # rows in any order, a loop and a duplicate
    ip = cin.adj_indptr.astype(np.int64)
    idx = cin.adj_indices.copy()
    for v in range(160):
        idx[ip[v]:ip[v + 1]] = idx[ip[v]:ip[v + 1]][::-1]
    v = int(np.flatnonzero(np.diff(ip) >= 3)[0])
    idx[ip[v]], idx[ip[v] + 1] = v, idx[ip[v] + 2]
    sh.adj_indices = idx
    _check(sh, sources)


@pytest.mark.parametrize("n", [1, 5, 64, 130])
def test_plan_without_entries_answers_from_one_launch(gpu, n):
    empty = _csr(n, [], [])
    plan = capi.SpMVPlan(n, n, empty.adj_indptr, empty.adj_indices, empty.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    for sources in ([0], [n - 1, 0, n // 2], [0, 0]):
        want = msbfs_model(empty, sources)
        for _ in range(2):
            got = _msbfs(plan, n, sources)
            _compare(got, want)
            assert got[5] == (0, 1 if len(set(sources)) == 1 else 0, 1, 0) and not got[0].any() and not got[2].any()
            assert np.count_nonzero(got[3] == 0) == len(sources) and np.count_nonzero(got[3] == NONE) == len(sources) * (n - 1)
    into = (np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.arange(n) / 3.0)
    got = _msbfs(plan, n, [0], into)                                   # accumulate: the three arrays stay as they are
    assert np.array_equal(got[0], into[0]) and np.array_equal(got[1], into[1]) and np.array_equal(got[2], bits64(into[2]))


@pytest.mark.parametrize("n", [1, 2, 63, 65, 130])
def test_sizes_that_are_no_multiple_of_64(gpu, n):
    if n == 1:
        ring = _csr(1, [0], [0])                                       # one vertex, a loop: an entry, but no edge to anybody else
    elif n == 2:
        ring = _sym_path(2, 2)
    else:
        s = np.arange(n - 1)
        ring = io.symmetrize_simple(_csr(n, np.concatenate([s + 1, [0]]), np.concatenate([s, [n - 1]])))[0]
    sources = sorted({0, n - 1, n // 2, n // 3})
    got = _check(ring, sources)
    assert got[5][1] == n                                             # connected: every vertex meets every source


def test_accumulate_over_two_calls_is_one_run_over_all_sources(gpu):
    cin = closeness_case("random_160")[0]
    plan = _bool_plan(cin)
    rng = np.random.default_rng(3)
    sources = rng.permutation(160)[:100].tolist()
    first = _msbfs(plan, 160, sources[:64])
    second = _msbfs(plan, 160, sources[64:], into=(first[0], first[1], first[2].view(np.float64)))
    far, reach, harmonic, hops, stats, _ = closeness_model(cin, sources)
    assert np.array_equal(second[0], far) and np.array_equal(second[1], reach) and np.array_equal(second[2], bits64(harmonic))
    assert np.array_equal(np.concatenate([first[3], second[3]]), hops) and np.array_equal(np.concatenate([first[4], second[4]]), stats)
    again = _msbfs(plan, 160, sources[64:], into=(first[0], first[1], first[2].view(np.float64)))
    assert all(np.array_equal(a, b) for a, b in zip(again[:5], second[:5]))             # two runs: identical bits


def test_module_layer(gpu):
    cin = closeness_case("random_160")[0]
    mod = M.SpMVModule(M.num_hbm_channels, 1024, 256)
    mod.set_semiring(M.LogicalSemiring)
    mod.set_mask_type(M.kNoMask)
    mod.set_up_runtime()
    mod.load_and_format_matrix(cin.copy(), True)
    mod.send_matrix_host_to_device()
    n = mod.get_num_rows()
    sources = [1, 50, 159, 77]
    out = Out(n, 4)
    source_stats, stats = mod.msbfs(sources, out.far, out.reach, out.harmonic, False, out.hops)
    capi.sync()
    padded = io.CSRMatrix(n, n, cin.adj_data, cin.adj_indices, np.concatenate([cin.adj_indptr, np.full(n - 160, cin.adj_indptr[-1], np.uint32)]))
    _compare(out.read() + (source_stats, stats), msbfs_model(padded, sources))


# ------------------------------------------------------------------ the C++ driver
@pytest.mark.parametrize("count,reverse", [(0, 0), (0, 1), (5, 1)])
def test_cpp_driver_equals_the_python_driver(gpu, tmp_path, golden_dir, count, reverse):
    build_cpp_driver("closeness_driver.cpp")
    path = os.path.join(golden_dir, GOLDEN)
    r = subprocess.run([CLOSENESS_DRIVER, path, str(tmp_path), str(count), str(reverse)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ClosenessCentrality::run OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    d = _driver(path)
    sources = [(7 * i) % 44 for i in range(count)] if count else None
    want = d.run(sources, reverse=bool(reverse), hops=True)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_far.bin"), dtype=np.uint64), d.far_)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_reach.bin"), dtype=np.uint32), d.reach_)
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_harmonic.bin"), dtype=np.uint64), bits64(d.harmonic_))
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_closeness.bin"), dtype=np.uint64), bits64(want))
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_hops.bin"), dtype=np.uint32), d.hops_.ravel())
    assert np.array_equal(np.fromfile(str(tmp_path / "cpp_eccentricity.bin"), dtype=np.uint64), d.eccentricity_.astype(np.uint64))
    for line in ("symmetric: 0", "sources: %d" % len(d.sources_), "batches: %d" % d.batches_, "levels: %d" % d.levels_,
                 "diameter: %d" % d.diameter_, "radius: %d" % d.radius_, "center: %d" % len(d.center_), "periphery: %d" % len(d.periphery_)):
        assert line + "\n" in r.stdout, (line, r.stdout[-1000:])
