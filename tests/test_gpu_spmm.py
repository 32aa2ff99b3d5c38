"""GPU parity of SpMM (gl_spmm, SpMVPlan.spmm, SpMMModule) against app.validate_spmm, the plain numpy f64 statement of
include/graphlily_hip_spmm.h with its derived bounds (tests/test_spmm_cpu.py checks the validator).  The matrix is rectangular,
its rows' lengths sit on both sides of the cuts (spmm_cut = 8, spmm_wg = 300 here) and of the wavefront's 64- and 256-entry steps, with
columns drawn with repetition.  X, the mask and Y are bound with a leading dimension above k and start as guard words: every
word behind a row's k columns, in rows outside the shard and behind the block must still be the guard afterwards."""
import ctypes

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob

pytestmark = pytest.mark.gpu

CUT, WG, GUARD = 8, 300, np.float32(-12345.5)
LENS = [0, 1, CUT, CUT + 1, 63, 64, 65, 255, 256, 257, WG + 1]
KS = [1, 3, 4, 5, 16, 17, 64, 65, 256, 257]
SEMIRINGS = {"muladd": M.ArithmeticSemiring, "andor": M.LogicalSemiring, "addmin": M.TropicalSemiring}
MASK_TYPES = [M.kNoMask, M.kMaskWriteToZero, M.kMaskWriteToOne]
N_ROWS, N_COLS = 220, 97
BOOLEAN = capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    set_knob(monkeypatch, "spmm_cut", CUT)
    set_knob(monkeypatch, "spmm_wg", WG)


def _case(k, semiring, lens=LENS):
    """-> (A, X, mask): (+,x) signed and cancelling; (min,+) signed eighths, X with the semiring's zero and +-inf; (||,&&) a thin X"""
    rng = np.random.default_rng(1000 * k + semiring.op)
    indptr = np.concatenate([[0], np.cumsum(np.resize(lens, N_ROWS))])
    nnz = int(indptr[-1])
    if semiring.op == M.kMulAdd:
        a, x = rng.choice([-1.0, 1.0], nnz) * (1 + 1e-3 * rng.standard_normal(nnz)), 1 + 1e-3 * rng.standard_normal((N_COLS, k))
    elif semiring.op == M.kAddMin:
        a, x = rng.integers(-64, 65, nnz) / 8.0, rng.uniform(-50, 50, (N_COLS, k))
        x[rng.random(x.shape) < 0.5] = semiring.zero
        x[rng.random(x.shape) < 0.03] = np.inf
        x[rng.random(x.shape) < 0.03] = -np.inf
    else:
        a, x = np.zeros(nnz), rng.random((N_COLS, k)) < 0.02
    csr = io.CSRMatrix(N_ROWS, N_COLS, a.astype(np.float32), rng.integers(0, N_COLS, nnz).astype(np.uint32), indptr.astype(np.uint32))
    return csr, x.astype(np.float32), rng.integers(0, 2, (N_ROWS, k)).astype(np.float32)


def _block(values, n, k, ld):
    out = np.full((n + 1, ld), GUARD, np.float32)
    out[:n, :k] = values
    return out


def _run(k, semiring, mask_type, pad=4, rows=(0, N_ROWS), lens=LENS, drop=None, cuts=(CUT, WG)):
    """one SpMMModule run on guarded blocks, checked; -> (module, Y's buffer, Y with its guard words)"""
    csr, x, mask = _case(k, semiring, lens)
    mod = M.SpMMModule()
    mod.set_up_runtime()
    mod.set_semiring(semiring)
    mod.set_mask_type(mask_type)
    mod.set_row_shard(*rows)
    mod.load_and_format_matrix(csr)
    mod.send_matrix_host_to_device()
    if drop is not None:        # a plan that stores these entries with a zero value: column 0xffffffff in the row copy
        mod.plan_ = capi.SpMVPlan(N_ROWS, N_COLS, csr.adj_indptr, csr.adj_indices, (~drop).astype(np.float32), 0, N_ROWS, BOOLEAN)
    ld = k + pad
    y_buf = capi.DeviceBuffer.from_host(_block(GUARD, N_ROWS, k, ld))
    mod.bind_vectors_buf(capi.DeviceBuffer.from_host(_block(x, N_COLS, k, ld)), k, ld)
    mod.bind_mask_buf(capi.DeviceBuffer.from_host(_block(mask, N_ROWS, k, ld)), ld)
    mod.bind_results_buf(y_buf, ld)
    mod.run()
    got = y_buf.read(np.float32).reshape(N_ROWS + 1, ld)
    guard = np.ones(got.shape, bool)
    guard[rows[0]:rows[1], :k] = False
    assert np.all(got[guard] == GUARD), "a word outside the rows' k columns was written"
    n = np.diff(csr.adj_indptr.astype(np.int64))[rows[0]:rows[1]]
    short = n <= cuts[0]
    wave = ~short & (n <= cuts[1])
    paths = (short.sum(), wave.sum(), (~short & ~wave).sum()) if csr.nnz else (0, 0, 0)      # without entries no row takes a path
    assert mod.stats_ == paths + (-(-k // 256),)
    if drop is not None:
        kept = np.repeat(np.arange(N_ROWS), np.diff(csr.adj_indptr.astype(np.int64)))[~drop]
        csr = io.CSRMatrix(N_ROWS, N_COLS, csr.adj_data[~drop], csr.adj_indices[~drop], np.concatenate([[0], np.cumsum(np.bincount(kept, minlength=N_ROWS))]))
    assert app.validate_spmm(csr, x, got[:N_ROWS, :k], semiring, mask, mask_type, rows=rows) == (rows[1] - rows[0]) * k
    return mod, y_buf, got


@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
@pytest.mark.parametrize("k", KS)
def test_every_k_and_path(k, semiring):
    """(the mask type rotates with k and the semiring: all nine combinations occur); (+,x) gives the same bits twice"""
    s = sorted(SEMIRINGS).index(semiring)
    mod, y_buf, got = _run(k, SEMIRINGS[semiring], MASK_TYPES[(KS.index(k) + s) % 3])
    if semiring == "muladd":
        mod.run()
        assert np.array_equal(y_buf.read(np.uint32), got.view(np.uint32).ravel())


@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
@pytest.mark.parametrize("mask_type", MASK_TYPES)
def test_unaligned_leading_dimensions_take_the_dword_twin(semiring, mask_type):
    _run(16, SEMIRINGS[semiring], mask_type, pad=3)


@pytest.mark.parametrize("knob,cuts", [("spmm_vec", (CUT, WG)), ("spmm_short", (-1, WG)), ("spmm_wave", (CUT, CUT))])
def test_closed_paths_and_forced_dwords(monkeypatch, knob, cuts):
    set_knob(monkeypatch, knob, 0)
    _run(16, M.ArithmeticSemiring, M.kMaskWriteToOne, cuts=cuts)


@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
def test_row_shard_empty_matrix_and_marker_entries(semiring):
    s = SEMIRINGS[semiring]
    _run(65, s, M.kMaskWriteToZero, rows=(50, 170))
    _run(5, s, M.kMaskWriteToOne, lens=[0])
    nnz = int(np.resize(LENS, N_ROWS).sum())
    _run(17, s, M.kNoMask, drop=np.arange(nnz) % 3 == 1)


K = 8
REFUSALS = {
    "null x": lambda b: dict(x=None), "null y": lambda b: dict(y=None), "k = 0": lambda b: dict(k=0), "ldx < k": lambda b: dict(ldx=K - 1),
    "ldy < k": lambda b: dict(ldy=K - 1), "ldm < k": lambda b: dict(ldm=K - 1, mask_type=1), "no mask": lambda b: dict(mask=None, mask_type=2),
    "mask type": lambda b: dict(mask_type=3), "op": lambda b: dict(op=3), "null a_val": lambda b: dict(a_val=None),
    "y over x": lambda b: dict(y=b["x"]), "y over mask": lambda b: dict(y=b["mask"], mask_type=1),
}


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["null plan", "no row copy"])
def test_refusals(what):
    capi.init(0)
    csr, x, mask = _case(K, M.ArithmeticSemiring, lens=[3])
    ones = np.ones(csr.adj_indices.shape[0], np.float32)
    plan = capi.SpMVPlan(N_ROWS, N_COLS, csr.adj_indptr, csr.adj_indices, ones, 0, N_ROWS, 0 if what == "no row copy" else BOOLEAN)
    b = dict(a_val=capi.DeviceBuffer.from_host(csr.adj_data), x=capi.DeviceBuffer.from_host(x),
             mask=capi.DeviceBuffer.from_host(mask), y=capi.DeviceBuffer(4 * N_ROWS * K), k=K, op=0, zero=0.0)
    if what == "null plan":
        code = capi.lib().gl_spmm(None, None, ctypes.c_void_p(b["x"].ptr), K, None, K, ctypes.c_void_p(b["y"].ptr), K, K, 0, 0.0, 0, None)
        assert code == capi.GL_ERR_INVALID_ARG
        return
    b.update(REFUSALS[what](b) if what in REFUSALS else {})
    with pytest.raises(capi.GraphLilyError) as e:
        plan.spmm(**b)
    assert e.value.code == (capi.GL_ERR_UNSUPPORTED if what == "no row copy" else capi.GL_ERR_INVALID_ARG)
