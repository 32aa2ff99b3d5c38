"""CPU suite of PageRank.solve (gl_pagerank_begin / gl_pagerank_update, app.PageRank.solve, graphlily::app::PageRank::solve):
the exports and their bindings exist, the numpy statement of the definition (kept here,
tests/test_gpu_pagerank_solve.py compares the drivers with it) conserves mass and contracts on the eight cases the GPU file runs,
the driver's host half (personalisation, dangling bits, what load records) agrees with it, every misuse is refused before any
device work, and the C++ driver compiles against include/ and fails loudly without a GPU.

The stop test: with K the first 0-based index at which the definition's residual drops below 1e-3, r[K + 1] < r[K] / 1.4
(asserted here), so tol = sqrt(r[K] * r[K + 1]) lies a factor >= sqrt(1.4) = 1.18 from both neighbouring residuals -- both
above 1e-4 / 1.4 -- while float noise in an L1 change of a unit-mass vector is of order 1e-7: every implementation of the
definition stops after K + 2 iterations."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M
from graphlily_amd.dist import EmulatedComm

from helpers import build_cpp_driver
from test_sssp_parents_cpu import GRAPHS, ROOT, raw_graph

PAGERANK_DRIVER = os.path.join(ROOT, "build", "pagerank_solve_driver")
DAMPING = 0.85
KINDS = ["uniform", "seeded"]
PADDED = {"uniform_3000": 3072, "rmat_4000": 4096, "rmat_sym_4000": 4096, "rmat_sym_6016": 6016}
REAL_DANGLING = {"uniform_3000": 65, "rmat_4000": 1502, "rmat_sym_4000": 1355, "rmat_sym_6016": 1818}
LONG = 16                       # iterations of the shared definition run (K + 2 <= 15)


def pagerank_by_definition(csr, damping, p, tol, max_iterations, each=None):
    """The definition, in numpy, on the PREPARED matrix `csr` (padded, M[v, u] = float(damping) * float(1 / outdeg(u))) and the
    personalisation p (float32[n]):
        x_0 = p;  dangle_k = f64 sum of x_k over the columns without a stored entry;
        c_k = float32((1.0 - d) + d * dangle_k) with d = float(float32(damping));
        y = M x_k with f64 row sums stored as float32;  x_{k+1} = fl32(y + fl32(c_k * p));  r_{k+1} = f64 sum |x_{k+1} - x_k|
    until r <= tol or max_iterations -> (x, residuals, iterations, converged).  each(k, x): called after iteration k (from 1)."""
    n = csr.num_rows
    assert csr.num_cols == n and p.dtype == np.float32 and p.shape == (n,)
    indptr = np.asarray(csr.adj_indptr).astype(np.int64)
    cols = np.asarray(csr.adj_indices).astype(np.int64)
    w = np.asarray(csr.adj_data, dtype=np.float32).astype(np.float64)
    lens = np.diff(indptr)
    dangling = np.bincount(cols, minlength=n) == 0
    d = float(np.float32(damping))
    x = p.copy()
    residuals = []
    for k in range(1, max_iterations + 1):
        dangle = float(x[dangling].astype(np.float64).sum())
        c = np.float32((1.0 - d) + d * dangle)
        prod = np.append(w * x[cols].astype(np.float64), 0.0)                   # (+ a sentinel: reduceat needs valid starts)
        y = np.where(lens > 0, np.add.reduceat(prod, indptr[:n]), 0.0).astype(np.float32)
        t = c * p                                                               # float32 * float32
        assert t.dtype == np.float32
        new = y + t
        assert new.dtype == np.float32
        residuals.append(float(np.abs(new.astype(np.float64) - x.astype(np.float64)).sum()))
        x = new
        if each is not None:
            each(k, x)
        if residuals[-1] <= tol:
            return x, np.array(residuals, np.float64), k, True
    return x, np.array(residuals, np.float64), max_iterations, False


@functools.lru_cache(maxsize=None)
def prepared_graph(name):
    """What PageRank.load_and_format_matrix(raw_graph(name), DAMPING) prepares, made here from the io functions -- shared, never
    modified"""
    m = raw_graph(name)
    n0 = m.num_rows
    io.util_round_csr_matrix_dim(m, 128, 128)
    io.util_normalize_csr_matrix_by_outdegree(m)
    m.adj_data = (m.adj_data * np.float32(DAMPING)).astype(np.float32)
    return m, n0


@functools.lru_cache(maxsize=None)
def given_personalization(name, kind):
    """What a caller passes as `personalization`: None, or 17 seed vertices with weights random + 0.1 (float64[n0])"""
    if kind == "uniform":
        return None
    _, n0 = prepared_graph(name)
    rng = np.random.default_rng(3)
    given = np.zeros(n0, np.float64)
    given[rng.choice(n0, size=17, replace=False)] = rng.random(17) + 0.1
    given.setflags(write=False)
    return given


@functools.lru_cache(maxsize=None)
def personalization(name, kind):
    """p of the definition: float32[n], 0 on padding, normalised in f64 before the cast"""
    m, n0 = prepared_graph(name)
    given = given_personalization(name, kind)
    p = np.zeros(m.num_rows, np.float64)
    p[:n0] = 1.0 / n0 if given is None else given / given.sum()
    p = p.astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def long_run(name, kind):
    """LONG iterations of the definition, never stopping (tol < 0: in float32 the iteration can reach its fixed point exactly,
    r = 0, within a few dozen iterations) -> (residuals, K, tol of the stop test, the sum over the real vertices and
    the largest padding entry after every iteration)"""
    m, n0 = prepared_graph(name)
    sums, pads = [], []

    def each(k, x):
        sums.append(float(x[:n0].astype(np.float64).sum()))
        pads.append(float(np.abs(x[n0:]).max(initial=0.0)))

    _, r, iterations, converged = pagerank_by_definition(m, DAMPING, personalization(name, kind), -1.0, LONG, each)
    assert iterations == LONG and not converged
    K = int(np.flatnonzero(r < 1e-3)[0])
    return r, K, float(np.sqrt(r[K] * r[K + 1])), np.array(sums), np.array(pads)


@functools.lru_cache(maxsize=None)
def reference(name, kind, tol, max_iterations):
    """(x, residuals, iterations, converged) by the definition -- shared, never modified"""
    m, _ = prepared_graph(name)
    x, r, iterations, converged = pagerank_by_definition(m, DAMPING, personalization(name, kind), tol, max_iterations)
    x.setflags(write=False)
    r.setflags(write=False)
    return x, r, iterations, converged


def loaded(name):
    pr = app.PageRank(M.num_hbm_channels, 1024, 256)
    pr.load_and_format_matrix(raw_graph(name), DAMPING)
    return pr


def test_library_exports_and_binds_gl_pagerank():
    L = capi.lib()
    for sym, nargs in (("gl_pagerank_ctl_bytes", 2), ("gl_pagerank_begin", 6), ("gl_pagerank_update", 9)):
        assert hasattr(L, sym), "libgraphlily_hip.so does not export %s" % sym
        assert sym in capi.EXPORTS
        assert getattr(L, sym).argtypes is not None and len(getattr(L, sym).argtypes) == nargs
    for cls, names in ((capi, ("pagerank_ctl_bytes", "pagerank_begin", "pagerank_update")), (app.PageRank, ("solve",))):
        for name in names:
            assert callable(getattr(cls, name))
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "graphlily_hip.h")).read())
    assert "int gl_pagerank_ctl_bytes(uint32_t slots, size_t *bytes);" in header
    assert ("int gl_pagerank_begin(const float *d_p, uint32_t n, const uint32_t *d_dangling_bits, float *d_x, void *d_ctl, "
            "uint32_t slots);") in header
    assert ("int gl_pagerank_update(float *d_y_inout, const float *d_x, const float *d_p, const uint32_t *d_dangling_bits, "
            "uint32_t n, float damping, double tol, void *d_ctl, uint32_t slot);") in header
    makefile = open(os.path.join(ROOT, "graphlily_amd", "csrc", "Makefile")).read()
    assert "gl_pagerank.hip" in makefile


def test_control_block_size_needs_no_device_and_grows_with_the_slots():
    one, hundred = capi.pagerank_ctl_bytes(1), capi.pagerank_ctl_bytes(100)
    assert hundred - one == 99 * 16                                 # one dangle and one residual word per slot
    assert one > capi.pagerank_ctl_head_bytes(1) == 48 and hundred % 8 == 0
    for bad in (0, capi.GL_PAGERANK_MAX_SLOTS + 1):
        with pytest.raises(capi.GraphLilyError) as e:
            capi.pagerank_ctl_bytes(bad)
        assert e.value.code == capi.GL_ERR_INVALID_ARG
    done, iterations, dangle, r = capi.pagerank_ctl_unpack(
        np.concatenate([np.array([1, 3, 4, 0], np.uint32).view(np.uint8), np.arange(10, dtype=np.float64).view(np.uint8),
                        np.zeros(64, np.uint8)]), 4)
    assert done and iterations == 3 and dangle.tolist() == [0, 1, 2, 3, 4] and r.tolist() == [5, 6, 7, 8, 9]


def test_compute_entry_points_fail_loudly_without_a_gpu():
    L = capi.lib()
    assert hasattr(L, "gl_pagerank_begin") and hasattr(L, "gl_pagerank_update")
    if capi.device_count() == 0:
        assert L.gl_pagerank_begin(None, 1, None, None, None, 1) == capi.GL_ERR_NOT_INITIALIZED
        assert L.gl_pagerank_update(None, None, None, None, 1, 0.85, 1e-6, None, 1) == capi.GL_ERR_NOT_INITIALIZED


@pytest.mark.parametrize("name", GRAPHS)
def test_load_records_what_solve_needs(name):
    m, n0 = prepared_graph(name)
    pr = loaded(name)
    assert pr.n_ == m.num_rows == PADDED[name] and pr.n_real_ == n0 == raw_graph(name).num_rows and pr.damping_ == DAMPING
    got = pr.SpMV_.csr_matrix_
    assert got.adj_indptr.tobytes() == m.adj_indptr.tobytes() and got.adj_indices.tobytes() == m.adj_indices.tobytes()
    assert got.adj_data.tobytes() == m.adj_data.tobytes()
    dangling = np.bincount(m.adj_indices, minlength=m.num_rows) == 0
    assert int(dangling[:n0].sum()) == REAL_DANGLING[name] and dangling[n0:].all()
    bits = pr._dangling_bits()
    assert bits.dtype == np.uint32 and bits.shape == ((m.num_rows + 31) // 32,)
    v = np.arange(m.num_rows)
    assert np.array_equal(((bits[v >> 5] >> (v & 31).astype(np.uint32)) & 1).astype(bool), dangling)
    for kind in KINDS:
        given = given_personalization(name, kind)
        p = pr._personalization(given)
        assert p.dtype == np.float32 and np.array_equal(p, personalization(name, kind))
        if given is not None:                                       # the padded length is accepted too
            assert np.array_equal(pr._personalization(np.concatenate([given, np.zeros(m.num_rows - n0)])), p)
            assert np.count_nonzero(p) == 17 and abs(float(p.astype(np.float64).sum()) - 1) < 1e-6
    # dangling vertices hold a visible share of the start mass: what pull() lets drain away
    share = float(personalization(name, "uniform")[dangling].astype(np.float64).sum())
    assert 0.02 < share < 0.39


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GRAPHS)
def test_definition_conserves_mass_and_contracts(name, kind):
    m, n0 = prepared_graph(name)
    r, K, tol, sums, pads = long_run(name, kind)
    assert np.all(np.abs(sums - 1) <= 1e-6), "the real vertices hold the whole mass after every iteration"
    assert np.all(pads == 0), "padding vertices hold exactly 0"
    assert 6 <= K <= 13
    assert r[K + 1] < r[K] / 1.4
    assert r[K + 1] * 1.18 < tol < r[K] / 1.18                      # (sqrt(1.4) = 1.183)
    # the stop test: K + 2 iterations, counted from 1
    x, rr, iterations, converged = reference(name, kind, tol, 60)
    assert converged and iterations == K + 2 and rr.shape == (K + 2,) and np.array_equal(rr, r[:K + 2])
    assert rr[-1] <= tol < rr[-2]
    # cut short
    x5, r5, it5, conv5 = reference(name, kind, 0.0, 5)
    assert it5 == 5 and not conv5 and np.array_equal(r5, r[:5]) and not np.array_equal(x5, x)
    if kind == "seeded":
        xu = reference(name, "uniform", long_run(name, "uniform")[2], 60)[0]
        seeds = np.flatnonzero(personalization(name, kind))
        assert float(x[seeds].sum()) > 10 * float(xu[seeds].sum()), "the seeds rank far higher than under uniform teleport"


MISUSE = [
    ("damping", dict(damping=0.5), "damping"),
    ("tol", dict(tol=-1e-9), "tol"),
    ("tol nan", dict(tol=float("nan")), "tol"),
    ("max_iterations", dict(max_iterations=0), "max_iterations"),
    ("check_every", dict(check_every=0), "check_every"),
    ("shape", dict(personalization=np.ones(7)), "shape"),
    ("shape 2d", dict(personalization=np.ones((3000, 1))), "shape"),
    ("negative", dict(personalization=-np.ones(3000)), "negative or non-finite"),
    ("nan", dict(personalization=np.full(3000, np.nan)), "negative or non-finite"),
    ("inf", dict(personalization=np.full(3000, np.inf)), "negative or non-finite"),
    ("zero sum", dict(personalization=np.zeros(3000)), "zero sum"),
    ("padding", dict(personalization=np.ones(3072)), "padding"),
]


@pytest.mark.parametrize("what,kwargs,match", MISUSE, ids=[m[0] for m in MISUSE])
def test_solve_refuses_misuse_before_any_device_work(what, kwargs, match):
    pr = loaded("uniform_3000")                 # loaded, never sent to a device: a check that came late would fail differently
    args = dict(damping=DAMPING, tol=1e-6, max_iterations=10, personalization=None, check_every=4)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        pr.solve(**args)


def test_solve_refuses_row_shards():
    pr = app.PageRank(M.num_hbm_channels, 1024, 256, comm=EmulatedComm(0, 2))
    pr.load_and_format_matrix(raw_graph("uniform_3000"), DAMPING)
    assert pr.r1_ - pr.r0_ < pr.n_
    with pytest.raises(NotImplementedError, match="row shards"):
        pr.solve(DAMPING)
    with pytest.raises(ValueError, match="tol"):       # (misuse is still misuse)
        pr.solve(DAMPING, tol=-1)


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    build_cpp_driver("pagerank_solve_driver.cpp")
    if capi.device_count() == 0:
        r = subprocess.run([PAGERANK_DRIVER, str(tmp_path / "none.npz"), str(tmp_path), "0.85", "1e-6", "10"],
                           capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
