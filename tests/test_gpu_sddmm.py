"""GPU parity of SDDMM (gl_sddmm, SpMVPlan.sddmm, SDDMMModule) against app.validate_sddmm, the plain numpy f64 statement of
include/graphlily_hip_sddmm.h with its derived bounds (tests/test_sddmm_cpu.py checks the validator).  The matrix is rectangular,
its rows' lengths sit on both sides of the cut (sddmm_cut = 8 here), of the piece path's 64-entry step and of one, two and four
pieces (sddmm_piece = 64), with columns drawn with repetition.  X and Y are bound with a leading dimension above k, `out` sits
between guard words: every guard word must be unchanged afterwards.  This file also holds gl_sddmm's shared-state cases (one
plan shared with gl_spmm, lists cached under other knobs): it is no caller of the shared row walk."""
import ctypes

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob

pytestmark = pytest.mark.gpu

CUT, PIECE, GUARD, FRONT = 8, 64, np.float32(-12345.5), 8
LENS = [0, 1, CUT, CUT + 1, 63, 64, 65, 129, 257]
KS = [1, 3, 4, 5, 16, 17, 64, 65, 256, 257, 1025, 1029]
SEMIRINGS = {"muladd": M.ArithmeticSemiring, "andor": M.LogicalSemiring, "addmin": M.TropicalSemiring}
N_ROWS, N_COLS = 220, 97
BOOLEAN = capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    set_knob(monkeypatch, "sddmm_cut", CUT)
    set_knob(monkeypatch, "sddmm_piece", PIECE)


def _case(k, semiring, lens=LENS):
    """-> (A, X, Y): (+,x) signed and cancelling over the features; (min,+) signed eighths in A, a finite X, Y with the semiring's
    zero and +-inf; (||,&&) thin X and Y (about one entry in two meets somewhere)"""
    rng = np.random.default_rng(1000 * k + semiring.op)
    indptr = np.concatenate([[0], np.cumsum(np.resize(lens, N_ROWS))])
    nnz = int(indptr[-1])
    if semiring.op == M.kMulAdd:
        a = rng.choice([-1.0, 1.0], nnz) * (1 + 1e-3 * rng.standard_normal(nnz))
        x, y = 1 + 1e-3 * rng.standard_normal((N_ROWS, k)), rng.choice([-1.0, 1.0], (N_COLS, k)) * (1 + 1e-3 * rng.standard_normal((N_COLS, k)))
    elif semiring.op == M.kAddMin:
        a, x, y = rng.integers(-64, 65, nnz) / 8.0, rng.uniform(-50, 50, (N_ROWS, k)), rng.uniform(-50, 50, (N_COLS, k))
        y[rng.random(y.shape) < 0.5] = semiring.zero
        y[rng.random(y.shape) < 0.03] = np.inf
        y[rng.random(y.shape) < 0.03] = -np.inf
    else:
        p = min(0.7, (0.7 / k) ** 0.5)
        a, x, y = np.zeros(nnz), rng.random((N_ROWS, k)) < p, rng.random((N_COLS, k)) < p
    csr = io.CSRMatrix(N_ROWS, N_COLS, a.astype(np.float32), rng.integers(0, N_COLS, nnz).astype(np.uint32), indptr.astype(np.uint32))
    return csr, x.astype(np.float32), y.astype(np.float32)


def _block(values, n, k, ld):
    out = np.full((n + 1, ld), GUARD, np.float32)
    out[:n, :k] = values
    return out


def _paths(csr, rows, cut, piece):
    n = np.diff(csr.adj_indptr.astype(np.int64))[rows[0]:rows[1]]
    return int(((n > 0) & (n <= cut)).sum()), int((-(-n[n > cut] // piece)).sum())


def _run(k, semiring, scaled, pad=4, rows=(0, N_ROWS), lens=LENS, drop=None, cut=CUT, piece=PIECE):
    """one SDDMMModule run on guarded blocks, checked; -> (module, the scores' bits, what the run was made of)"""
    csr, x, y = _case(k, semiring, lens)
    mod = M.SDDMMModule()
    mod.set_up_runtime()
    mod.set_semiring(semiring)
    mod.set_scaled(scaled)
    mod.set_row_shard(*rows)
    mod.load_and_format_matrix(csr)
    mod.send_matrix_host_to_device()
    if drop is not None:        # a plan that stores these entries with a zero value: column 0xffffffff in the row copy
        mod.plan_ = capi.SpMVPlan(N_ROWS, N_COLS, csr.adj_indptr, csr.adj_indices, (~drop).astype(np.float32), 0, N_ROWS, BOOLEAN)
        csr = io.CSRMatrix(N_ROWS, N_COLS, csr.adj_data, np.where(drop, 0xffffffff, csr.adj_indices).astype(np.uint32), csr.adj_indptr)
    ld, count = k + pad, mod.count_
    x_buf, y_buf = capi.DeviceBuffer.from_host(_block(x, N_ROWS, k, ld)), capi.DeviceBuffer.from_host(_block(y, N_COLS, k, ld))
    whole = capi.DeviceBuffer.from_host(np.full(count + 2 * FRONT, GUARD, np.float32))
    mod.bind_features_bufs(x_buf, y_buf, k, ld, ld)
    mod.bind_results_buf(capi.DeviceBuffer(4 * count, ptr=whole.ptr + 4 * FRONT, keepalive=whole))
    mod.run()
    got = whole.read(np.float32)
    assert np.all(got[:FRONT] == GUARD) and np.all(got[FRONT + count:] == GUARD), "a word outside the entries' was written"
    for buf, n in ((x_buf, N_ROWS), (y_buf, N_COLS)):
        assert np.all(buf.read(np.float32).reshape(n + 1, ld)[:, k:] == GUARD) and np.all(buf.read(np.float32)[n * ld:] == GUARD)
    assert mod.stats_ == _paths(csr, rows, cut, piece) + (-(-k // 256),)
    assert app.validate_sddmm(csr, x, y, got[FRONT:FRONT + count], semiring, scaled, rows=rows) == count
    return mod, got.view(np.uint32), (csr, x, y, whole)


@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
@pytest.mark.parametrize("k", KS)
def test_every_k_and_path(k, semiring):
    """(`scaled` alternates with the index); (+,x) gives the same bits twice"""
    mod, bits, keep = _run(k, SEMIRINGS[semiring], (KS.index(k) + sorted(SEMIRINGS).index(semiring)) % 2 == 0)
    if semiring == "muladd":
        mod.run()
        assert np.array_equal(keep[3].read(np.uint32), bits)


@pytest.mark.parametrize("knob,value,k", [(knob, value, k) for k in (17, 65) for knob, value in (("sddmm_short", 0), ("sddmm_vec", 0), ("sddmm_piece", 256))] +
                         [("sddmm_vec", 0, 1028)])         # (1028 + 4 is a multiple of 4: the LDS-staged kernel's 16-byte loads)
def test_the_bits_depend_on_no_path(monkeypatch, k, knob, value):
    _, bits, _ = _run(k, M.ArithmeticSemiring, True)
    set_knob(monkeypatch, knob, value)
    _, other, _ = _run(k, M.ArithmeticSemiring, True, cut=-1 if knob == "sddmm_short" else CUT, piece=value if knob == "sddmm_piece" else PIECE)
    assert np.array_equal(bits, other)


@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
def test_unaligned_leading_dimensions_take_the_dword_twin(semiring):
    _run(16, SEMIRINGS[semiring], True, pad=3)


@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
def test_row_shard_empty_matrix_and_marker_entries(semiring):
    s = SEMIRINGS[semiring]
    _run(65, s, True, rows=(50, 170))
    _run(5, s, False, lens=[0])
    nnz = int(np.resize(LENS, N_ROWS).sum())
    _run(17, s, True, drop=np.arange(nnz) % 3 == 1)


K = 8
REFUSALS = {
    "null x": lambda b: dict(x=None), "null y": lambda b: dict(y=None), "null out": lambda b: dict(out=None), "k = 0": lambda b: dict(k=0),
    "ldx < k": lambda b: dict(ldx=K - 1), "ldy < k": lambda b: dict(ldy=K - 1), "op": lambda b: dict(op=3),
    "out over x": lambda b: dict(out=b["x"]), "out over y": lambda b: dict(out=b["y"]), "out over a_val": lambda b: dict(out=b["a_val"]),
}


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["null plan", "no row copy"])
def test_refusals(what):
    capi.init(0)
    csr, x, y = _case(K, M.ArithmeticSemiring, lens=[3])
    ones = np.ones(csr.adj_indices.shape[0], np.float32)
    plan = capi.SpMVPlan(N_ROWS, N_COLS, csr.adj_indptr, csr.adj_indices, ones, 0, N_ROWS, 0 if what == "no row copy" else BOOLEAN)
    b = dict(a_val=capi.DeviceBuffer.from_host(csr.adj_data), x=capi.DeviceBuffer.from_host(x), y=capi.DeviceBuffer.from_host(y),
             out=capi.DeviceBuffer(4 * csr.nnz), k=K, op=0, zero=0.0)
    if what == "null plan":
        p = lambda buf: ctypes.c_void_p(buf.ptr)
        assert capi.lib().gl_sddmm(None, None, p(b["x"]), K, p(b["y"]), K, p(b["out"]), K, 0, 0.0, None) == capi.GL_ERR_INVALID_ARG
        return
    b.update(REFUSALS[what](b) if what in REFUSALS else {})
    with pytest.raises(capi.GraphLilyError) as e:
        plan.sddmm(**b)
    assert e.value.code == (capi.GL_ERR_UNSUPPORTED if what == "no row copy" else capi.GL_ERR_INVALID_ARG)


def test_one_plan_shared_with_spmm_and_lists_of_other_knobs(monkeypatch):
    """sddmm, then spmm on the same plan, then sddmm under other knobs (the lists are rebuilt) and under the first ones again
    (rebuilt once more): every result is checked by its validator, and every sddmm gives the first one's bits"""
    k = 16
    mod, bits, (csr, x, y, whole) = _run(k, M.ArithmeticSemiring, True, pad=0)
    z = np.random.default_rng(5).standard_normal((N_COLS, k)).astype(np.float32)
    z_buf, agg = capi.DeviceBuffer.from_host(z), capi.DeviceBuffer(4 * N_ROWS * k)
    mod.plan_.spmm(mod.a_val_buf, z_buf, agg, k, M.kMulAdd, 0.0)
    assert app.validate_spmm(csr, z, agg.read(np.float32).reshape(N_ROWS, k), M.ArithmeticSemiring) == N_ROWS * k
    for cut, piece in ((20, 128), (CUT, PIECE)):
        set_knob(monkeypatch, "sddmm_cut", cut)
        set_knob(monkeypatch, "sddmm_piece", piece)
        capi.fill_f32(mod.results_buf, 0.0, mod.count_)
        mod.run()
        assert mod.stats_ == _paths(csr, (0, N_ROWS), cut, piece) + (1,)
        assert np.array_equal(whole.read(np.uint32), bits)


def test_scores_feed_spmm_on_the_device():
    """Y = (A o X Y^T) Z: SDDMMModule.results_buf is SpMMModule's a_val_buf, no host round trip; checked by validate_spmm with
    the read-back scores as A's values (the scores themselves by validate_sddmm, in _run)"""
    k = 16
    edge, _, (csr, x, y, whole) = _run(k, M.ArithmeticSemiring, True)
    z = np.random.default_rng(6).standard_normal((N_COLS, k)).astype(np.float32)
    agg = M.SpMMModule()
    agg.set_up_runtime()
    agg.load_and_format_matrix(csr)
    agg.send_matrix_host_to_device()
    agg.a_val_buf = edge.results_buf
    agg.send_vectors_host_to_device(z)
    agg.run()
    scored = io.CSRMatrix(N_ROWS, N_COLS, edge.send_results_device_to_host().adj_data, csr.adj_indices, csr.adj_indptr)
    assert app.validate_spmm(scored, z, agg.send_results_device_to_host(), M.ArithmeticSemiring) == N_ROWS * k
