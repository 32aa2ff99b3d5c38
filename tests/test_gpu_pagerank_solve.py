"""GPU suite of PageRank.solve (gl_pagerank_begin / gl_pagerank_update, app.PageRank.solve, graphlily::app::PageRank::solve)
against the numpy statement of the definition in tests/test_pagerank_solve_cpu.py.

The kernels alone: x = p and x_new = fl32(y + fl32(c * p)) are compared bit for bit (c formed from the dangling sum the device
reported, which is itself checked first), the two f64 sums to relative n * 2^-52 -- the worst case of reordering a sum of n
non-negative terms -- and repeated calls, unaligned pointers and frozen updates bit for bit.

The drivers, on four graphs x {uniform, 17 seeds}: the iteration count is the definition's K + 2 exactly, ranks are within
1e-5 * want on every vertex (the project's float bar; exact zeros stay exact), padding is 0, the ranks sum to 1 within 1e-6.
The residual history differs from the definition's only by rounding noise (the device's SpMV adds a row in another order than
numpy's f64 reduceat before both round to float32).  Measured on one MI355X, the largest relative deviation of residuals_ from
the definition's is 1.385e-05 over the eight cases (rmat_sym_6016 uniform; the other seven lie between 1.5e-06 and 8.8e-06,
EXPERIMENTS.md Round 10); asserted is ten times that, RESIDUAL_BOUND below.  check_every, repetition and a pull() before and
after change nothing, bit for bit, and the C++ driver returns the Python driver's words."""
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, module as M

from helpers import build_cpp_driver
from test_sssp_parents_cpu import GRAPHS, raw_graph
from test_pagerank_solve_cpu import (DAMPING, KINDS, PAGERANK_DRIVER, given_personalization, long_run, personalization, prepared_graph,
                                     reference)

pytestmark = pytest.mark.gpu

# Largest relative deviation of residuals_ from the definition's over the eight cases, measured on one MI355X (EXPERIMENTS.md
# Round 10).  Asserted: 10 x that (rounding noise differs per graph and per plan layout), never looser than 1e-2.
RESIDUAL_MEASURED = 1.385e-5
RESIDUAL_BOUND = min(1e-2, 10 * RESIDUAL_MEASURED)

SIZES = [1, 63, 64, 257, 6016, 100003]
EPS52 = 2.0 ** -52


# ---- the kernels alone, through capi
def _inputs(n):
    rng = np.random.default_rng(1000 + n)
    x, y, p = (rng.random(n, dtype=np.float32) for _ in range(3))
    bits = rng.integers(0, 1 << 32, size=(n + 31) // 32, dtype=np.uint64).astype(np.uint32)    # (bits past n are set too)
    v = np.arange(n)
    marked = ((bits[v >> 5] >> (v & 31).astype(np.uint32)) & 1).astype(bool)
    return x, y, p, bits, marked


class _Run:
    """One control block and the device copies of one input set; `shift`: every float vector starts 4 bytes past a 16-byte
    boundary (the kernels' scalar path)"""

    def __init__(self, n, slots=3, shift=False):
        self.n, self.slots = n, slots
        self.x, self.y, self.p, self.bits, self.marked = _inputs(n)
        self.ctl = capi.DeviceBuffer.from_host(np.full(capi.pagerank_ctl_bytes(slots), 0xAB, np.uint8))     # (recycled memory)
        self.d_bits = capi.DeviceBuffer.from_host(self.bits)
        off = 4 if shift else 0
        self.bufs = {}
        for name in ("x", "y", "p", "out"):
            whole = capi.DeviceBuffer(4 * n + 16)
            self.bufs[name] = capi.DeviceBuffer(4 * n, ptr=whole.ptr + off, keepalive=whole)
            assert (self.bufs[name].ptr % 16 != 0) == shift
        self.bufs["p"].write(self.p)

    def head(self):
        capi.sync()
        return capi.pagerank_ctl_unpack(self.ctl.read(np.uint8), self.slots)

    def begin(self):
        capi.pagerank_begin(self.bufs["p"], self.n, self.d_bits, self.bufs["out"], self.ctl, self.slots)
        capi.sync()
        return self.bufs["out"].read(np.float32, self.n)

    def update(self, slot, tol, y=None):
        self.bufs["x"].write(self.x)
        self.bufs["y"].write(self.y if y is None else y)
        capi.pagerank_update(self.bufs["y"], self.bufs["x"], self.bufs["p"], self.d_bits, self.n, DAMPING, tol, self.ctl, slot)
        capi.sync()
        return self.bufs["y"].read(np.float32, self.n)


def _close(got, want, n):
    return abs(got - want) <= n * EPS52 * abs(want)


def _expected_update(run, dangle_before):
    d = float(np.float32(DAMPING))
    c = np.float32((1.0 - d) + d * dangle_before)
    new = run.y + c * run.p
    assert new.dtype == np.float32
    r = float(np.abs(new.astype(np.float64) - run.x.astype(np.float64)).sum())
    return new, r, float(new[run.marked].astype(np.float64).sum())


@pytest.mark.parametrize("shift", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_begin_and_update_against_numpy(gpu, n, shift):
    run = _Run(n, shift=shift)
    assert np.array_equal(run.begin().view(np.uint32), run.p.view(np.uint32)), "begin leaves x == p bit for bit"
    done, iterations, dangle, r = run.head()
    want0 = float(run.p[run.marked].astype(np.float64).sum())
    print("n=%d dangle_0: got %r want %r" % (n, dangle[0], want0))
    assert not done and iterations == 0 and _close(dangle[0], want0, n)
    assert not dangle[1:].any() and not r.any(), "the rest of the head is cleared"
    # one update, not converging (tol = 0)
    got = run.update(1, 0.0)
    new, want_r, want_dangle = _expected_update(run, dangle[0])
    assert np.array_equal(got.view(np.uint32), new.view(np.uint32)), "x_new == fl32(y + fl32(c * p)) bit for bit"
    done, iterations, dangle1, r1 = run.head()
    print("n=%d r_1: got %r want %r; dangle_1: got %r want %r" % (n, r1[1], want_r, dangle1[1], want_dangle))
    assert not done and iterations == 1
    assert _close(r1[1], want_r, n) and _close(dangle1[1], want_dangle, n)
    assert dangle1[0] == dangle[0] and not dangle1[2:].any() and not r1[2:].any() and r1[0] == 0
    # a second update, from dangle[1], that converges (any residual is <= 1e30) ...
    got2 = run.update(2, 1e30)
    new2, want_r2, want_dangle2 = _expected_update(run, dangle1[1])
    assert np.array_equal(got2.view(np.uint32), new2.view(np.uint32))
    done, iterations, dangle2, r2 = run.head()
    assert done and iterations == 2 and _close(r2[2], want_r2, n) and _close(dangle2[2], want_dangle2, n)
    # ... after which an update copies x to its output and changes nothing else
    before = run.ctl.read(np.uint8)
    got3 = run.update(3, 0.0)
    assert np.array_equal(got3.view(np.uint32), run.x.view(np.uint32))
    capi.sync()
    assert np.array_equal(run.ctl.read(np.uint8), before)


@pytest.mark.parametrize("n", SIZES)
def test_calls_repeat_bit_for_bit_whatever_the_alignment(gpu, n):
    outs = []
    for shift in (False, False, True):
        run = _Run(n, shift=shift)
        x0 = run.begin()
        x1 = run.update(1, 0.0)
        head = run.ctl.read(np.uint8, capi.pagerank_ctl_head_bytes(run.slots))
        outs.append((x0.tobytes(), x1.tobytes(), head.tobytes()))
    assert outs[0] == outs[1], "two identical calls"
    assert outs[0] == outs[2], "the scalar path adds in the same order"


@pytest.mark.parametrize("n", SIZES)
def test_update_with_done_set_leaves_everything_in_place(gpu, n):
    run = _Run(n)
    run.begin()
    capi.sync()
    run.ctl.write(np.array([1], np.uint32))             # done, before any update ran
    before = run.ctl.read(np.uint8)
    got = run.update(1, 0.0)
    assert np.array_equal(got.view(np.uint32), run.x.view(np.uint32)), "the output is x"
    assert np.array_equal(run.ctl.read(np.uint8), before), "the control block is unchanged"


def test_a_slot_past_the_blocks_own_is_a_frozen_update(gpu):
    run = _Run(257, slots=2)
    run.begin()
    before = run.ctl.read(np.uint8)
    got = run.update(3, 0.0)                            # in [1, GL_PAGERANK_MAX_SLOTS], but the block has two slots
    assert np.array_equal(got, run.x) and np.array_equal(run.ctl.read(np.uint8), before)


def test_bad_arguments_are_refused(gpu):
    run = _Run(64)
    L = capi.lib()
    b = {k: capi._p(v) for k, v in run.bufs.items()}
    bits, ctl, null = capi._p(run.d_bits), capi._p(run.ctl), capi._p(None)
    bad_begin = [(null, 64, bits, b["out"], ctl, 3), (b["p"], 64, null, b["out"], ctl, 3), (b["p"], 64, bits, null, ctl, 3),
                 (b["p"], 64, bits, b["out"], null, 3), (b["p"], 0, bits, b["out"], ctl, 3), (b["p"], 64, bits, b["out"], ctl, 0),
                 (b["p"], 64, bits, b["out"], ctl, capi.GL_PAGERANK_MAX_SLOTS + 1), (b["p"], 64, bits, b["p"], ctl, 3)]
    for args in bad_begin:
        assert L.gl_pagerank_begin(*args) == capi.GL_ERR_INVALID_ARG, args
    ok = (b["y"], b["x"], b["p"], bits, 64, DAMPING, 0.0, ctl, 1)
    bad_update = [ok[:i] + (null,) + ok[i + 1:] for i in (0, 1, 2, 3, 7)]
    bad_update += [ok[:4] + (0,) + ok[5:], ok[:8] + (0,), ok[:8] + (capi.GL_PAGERANK_MAX_SLOTS + 1,), (b["x"],) + ok[1:]]
    for args in bad_update:
        assert L.gl_pagerank_update(*args) == capi.GL_ERR_INVALID_ARG, args
    with pytest.raises(capi.GraphLilyError, match="slot"):
        capi.pagerank_update(run.bufs["y"], run.bufs["x"], run.bufs["p"], run.d_bits, 64, DAMPING, 0.0, run.ctl, 0)
    run.begin()
    assert run.head()[1] == 0, "none of them ran"


# ---- the drivers
_DRIVERS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_drivers():
    """The drivers shared by this file's tests hold plans and vectors on the device; a block still out keeps its slab of the
    device pool, and the pieces parked in it, from being released -- the files that run after this one get the pool back as
    they would have found it (tests/test_gpu_runtime.py::test_pool_best_fit_and_slab_reset asserts which blocks of the
    pool its allocations are handed, and blocks of ours still out would stand among them)."""
    yield
    import gc
    _DRIVERS.clear()
    gc.collect()
    capi.pool_trim()


def _driver(name):
    if name not in _DRIVERS:
        pr = app.PageRank(M.num_hbm_channels, 1024, 256)
        pr.set_target("hw")
        pr.set_up_runtime("unused.xclbin")
        pr.load_and_format_matrix(raw_graph(name), DAMPING)
        pr.send_matrix_host_to_device()
        _DRIVERS[name] = pr
    return _DRIVERS[name]


def _check_ranks(got, want, n0, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.all(np.abs(got.astype(np.float64) - want) <= 1e-5 * want.astype(np.float64)), what    # (want == 0: got == 0)
    assert not got[n0:].any(), what + ": padding"
    assert abs(float(got.astype(np.float64).sum()) - 1) <= 1e-6, what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GRAPHS)
def test_solve_against_the_definition(gpu, name, kind):
    _, n0 = prepared_graph(name)
    _, K, tol, _, _ = long_run(name, kind)
    want, want_r, want_iterations, _ = reference(name, kind, tol, 60)
    assert want_iterations == K + 2
    pr = _driver(name)
    what = "%s, %s" % (name, kind)
    got = pr.solve(DAMPING, tol, 60, given_personalization(name, kind))
    both = min(len(want_r), len(pr.residuals_))
    deviation = float(np.max(np.abs(pr.residuals_[:both] - want_r[:both]) / want_r[:both]))
    print("%s: iterations %d (want %d), largest relative deviation of the residuals %.3e, of the ranks %.3e"
          % (what, pr.iterations_, K + 2, deviation,
             float(np.max(np.abs(got.astype(np.float64) - want)[want > 0] / want[want > 0]))))
    assert pr.iterations_ == K + 2 and pr.converged_ is True, what
    _check_ranks(got, want, n0, what)
    assert pr.residuals_.dtype == np.float64 and pr.residuals_.shape == (K + 2,), what
    assert deviation <= RESIDUAL_BOUND, what
    assert pr.residuals_[-1] <= tol < pr.residuals_[-2], what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GRAPHS[1::2])
def test_solve_does_not_depend_on_check_every_or_on_what_ran_before(gpu, name, kind):
    _, n0 = prepared_graph(name)
    _, K, tol, _, _ = long_run(name, kind)
    given = given_personalization(name, kind)
    pr = _driver(name)
    pulled = pr.pull(DAMPING, 10)
    runs = []
    for check_every in (1, 8, 8):                       # ... and two calls in a row
        x = pr.solve(DAMPING, tol, 60, given, check_every=check_every)
        runs.append((x.tobytes(), pr.residuals_.tobytes(), pr.iterations_, pr.converged_))
    assert runs[0] == runs[1], "check_every 1 and 8"
    assert runs[1] == runs[2], "two calls in a row"
    assert runs[0][2] == K + 2
    # tol = 0: max_iterations iterations, not converged
    want5, want_r5, _, _ = reference(name, kind, 0.0, 5)
    x5 = pr.solve(DAMPING, 0, 5, given)
    assert pr.iterations_ == 5 and pr.converged_ is False and pr.residuals_.shape == (5,)
    _check_ranks(x5, want5, n0, "%s, %s, 5 iterations" % (name, kind))
    assert np.all(np.abs(pr.residuals_ - want_r5) <= RESIDUAL_BOUND * want_r5)
    # a batch that would run past max_iterations does not
    r5 = pr.residuals_.copy()
    x7 = pr.solve(DAMPING, 0, 7, given, check_every=4)
    assert pr.iterations_ == 7 and not pr.converged_ and np.array_equal(pr.residuals_[:5], r5)
    assert not np.array_equal(x7, x5)
    # pull() is what it was: semiring, bindings and chain state are left alone
    assert pr.SpMV_.semiring_ is pr.semiring_
    again = pr.pull(DAMPING, 10)
    assert again.tobytes() == pulled.tobytes()


def test_reference_order_plans_run_the_same_sequence(gpu):
    name, kind = "rmat_4000", "seeded"
    _, n0 = prepared_graph(name)
    _, K, tol, _, _ = long_run(name, kind)
    pr = app.PageRank(M.num_hbm_channels, 1024, 256)
    pr.set_up_runtime("unused.xclbin")
    pr.SpMV_.set_plan_flags(capi.GL_PLAN_REFERENCE_ORDER)
    pr.load_and_format_matrix(raw_graph(name), DAMPING)
    pr.send_matrix_host_to_device()
    got = pr.solve(DAMPING, tol, 60, given_personalization(name, kind))
    assert pr.iterations_ == K + 2 and pr.converged_
    assert not got[n0:].any() and abs(float(got.astype(np.float64).sum()) - 1) <= 1e-6
    # that layout rounds every product and adds a row's products one after the other in float32: a row sum of k non-negative
    # terms is off by at most (k + 1) * 2^-24 of itself, the teleport term and the final add by two more roundings, and a
    # vertex the teleport does not reach inherits its neighbours' relative error in full: at worst the per-iteration error
    # adds up over the iterations run
    m, _ = prepared_graph(name)
    bound = pr.iterations_ * int(np.diff(m.adj_indptr.astype(np.int64)).max() + 3) * 2.0 ** -24
    want = reference(name, kind, tol, 60)[0].astype(np.float64)
    assert 1e-5 < bound < 1e-3 and np.all(np.abs(got - want) <= bound * want)


def test_cpp_driver_equals_the_python_driver(gpu, tmp_path):
    import scipy.sparse as sp
    if not os.path.exists(PAGERANK_DRIVER):
        build_cpp_driver("pagerank_solve_driver.cpp")
    name = "rmat_sym_4000"
    m = raw_graph(name)
    A = sp.csr_matrix((m.adj_data, m.adj_indices.astype(np.int32), m.adj_indptr.astype(np.int32)), shape=(m.num_rows, m.num_cols),
                      dtype=np.float32)
    path = str(tmp_path / "rmat_sym_csr_float32.npz")
    sp.save_npz(path, A, compressed=False)
    pr = _driver(name)
    tol = long_run(name, "uniform")[2]
    seeds = [5, 77, 1234, 3999]
    for s in ([], seeds):
        r = subprocess.run([PAGERANK_DRIVER, path, str(tmp_path), repr(DAMPING), repr(tol), "60"] + [str(v) for v in s],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "PageRank::solve OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
        given = None
        if s:
            given = np.zeros(m.num_rows)
            given[s] = 1
        want = pr.solve(DAMPING, tol, 60, given)
        assert pr.converged_ and ("iterations %d converged 1" % pr.iterations_) in r.stdout, r.stdout[-2000:]
        assert np.fromfile(str(tmp_path / "cpp_ranks.bin"), np.uint32).tobytes() == want.tobytes()
        assert np.fromfile(str(tmp_path / "cpp_residuals.bin"), np.float64).tobytes() == pr.residuals_.tobytes()
