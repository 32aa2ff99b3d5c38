"""GPU parity of SpGEMM (gl_spgemm_symbolic / gl_spgemm_numeric, SpMVPlan.spgemm_*, SpGEMMModule, app.TwoHop) against spgemm_model
of tests/test_spgemm_cpu.py (checked there against a dense numpy product).  Every test runs with the default paths, with
spgemm_wave=0 (no wavefront path) and with spgemm_lds=0 (every row in a slab); the boundary cases also shrink the tables to 64 and
256 slots.  Outputs start as garbage with guard words behind them, and every check is made twice: the second call runs from the
cached bins.  Integer-valued inputs, (min,+) and (||,&&) are compared with np.array_equal; signed reals under (+,x) to the
derived bound of include/graphlily_hip_spgemm.h, which app.validate_spgemm states.  This caller's contract cases (gl_rows.h) live
here."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import set_knob
from test_kcore_cpu import _csr as _csr_as_given
from test_spgemm_cpu import GOLDEN, MASKS, SEMIRINGS, SPGEMM_DRIVER, _csr, random_csr, spgemm_model

pytestmark = pytest.mark.gpu

G32 = 0xdeadbeef
GUARD = 64
MODES = {"default": {}, "no_wave": {"spgemm_wave": 0}, "all_in_slabs": {"spgemm_lds": 0}}
WAVE_SLOTS, LDS_SLOTS = 64, 256


@pytest.fixture(autouse=True, params=sorted(MODES))
def mode(request, monkeypatch):
    for key, value in MODES[request.param].items():
        set_knob(monkeypatch, key, value)
    return request.param


def _plan(m, r0=0, r1=None, flags=capi.GL_PLAN_BOOLEAN):
    return capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, np.ones(m.adj_indices.shape[0], np.float32), r0,
                         m.num_rows if r1 is None else r1, flags=flags)


def _values(m):
    return capi.DeviceBuffer.from_host(m.adj_data if m.adj_data.shape[0] else np.zeros(1, np.float32))


def _product(pa, pb, va, vb, n, op, mask=None, complement=False):
    """-> (C, symbolic stats, numeric stats); the guard words behind all three outputs must still be garbage"""
    indptr = capi.DeviceBuffer.from_host(np.full(n + 1 + GUARD, G32, np.uint32))
    sym = pa.spgemm_symbolic(pb, indptr, mask, complement)
    ip = indptr.read(np.uint32, n + 1 + GUARD)
    assert np.all(ip[n + 1:] == G32), "a guard word behind d_c_indptr was written"
    nnz = int(ip[n])
    assert ip[0] == 0 and nnz == sym[0]
    idx = capi.DeviceBuffer.from_host(np.full(nnz + GUARD, G32, np.uint32))
    val = capi.DeviceBuffer.from_host(np.full(nnz + GUARD, G32, np.uint32))
    num = pa.spgemm_numeric(pb, op, va, vb, indptr, idx, val, mask, complement, stats=True)
    i, v = idx.read(np.uint32, nnz + GUARD), val.read(np.uint32, nnz + GUARD)
    assert np.all(i[nnz:] == G32) and np.all(v[nnz:] == G32), "a guard word behind C was written"
    return io.CSRMatrix(n, n, v[:nnz].view(np.float32), i[:nnz], ip[:n + 1]), sym, num


def _bins(counts, mode, wave=512, lds=8192):
    """-> (rows in the workgroup path, rows in the slab path) for the rows' counts"""
    counts = counts[counts > 0]
    if mode == "all_in_slabs":
        return 0, int(counts.size)
    low = 0 if mode == "no_wave" else wave
    return int(np.count_nonzero((counts > low) & (counts <= lds))), int(np.count_nonzero(counts > lds))


def _check(a, b, op, mask=None, complement=False, mode="default", tables=(512, 8192), exact=True, what=""):
    pa = _plan(a)
    pb = pa if b is a else _plan(b)
    pm = None if mask is None else pa if mask is a else _plan(mask)
    va = _values(a)
    vb = va if b is a else _values(b)
    want, _ = spgemm_model(a, b, op, mask, complement)
    rows = np.repeat(np.arange(a.num_rows), np.diff(a.adj_indptr.astype(np.int64)))
    bounds = np.bincount(rows, np.diff(b.adj_indptr.astype(np.int64))[a.adj_indices], a.num_rows).astype(np.int64)   # the rows' products
    for call in range(2):
        c, sym, num = _product(pa, pb, va, vb, a.num_rows, op, pm, complement)
        assert np.array_equal(c.adj_indptr, want.adj_indptr) and np.array_equal(c.adj_indices, want.adj_indices), (what, call)
        if exact:
            assert np.array_equal(c.adj_data, want.adj_data), (what, call, "first difference at entry %d" % int(np.flatnonzero(c.adj_data != want.adj_data)[0]))
        else:
            app.validate_spgemm(a, b, c, op, mask, complement)
        ran = not (mask is not None and mask.nnz == 0 and not complement)      # (a mask that admits nothing: no row takes a path)
        assert sym == (want.nnz, int(bounds.sum())) + (_bins(bounds, mode, *tables) if ran else (0, 0)), (what, call)
        assert num == (want.nnz, int(bounds.sum())) + (_bins(np.diff(want.adj_indptr.astype(np.int64)), mode, *tables) if ran else (0, 0)), (what, call)
    return c


@functools.lru_cache(maxsize=None)
def row_case(kind, c):
    """-> (A, B): row 0 of A names rows of B that give c distinct columns -- `once`: d = min(c, 4) rows that share them out, at
    random places; `four`: four rows that each hold all of them; `chain`: as once, the columns all multiples of 256, which one
    slot of every table serves; `run`: as once, consecutive columns.  Row 5 of A names only empty rows of B, every other row of
    A is empty.  Small integer values."""
    rng = np.random.default_rng(c)
    n = 256 * (c + 2) if kind == "chain" else 1024
    cols = {"chain": 256 * np.arange(1, c + 1), "run": 300 + np.arange(c)}.get(kind)
    cols = np.sort(rng.choice(np.arange(16, n - 16), size=c, replace=False)) if cols is None else cols
    d = 4 if kind == "four" else min(c, 4)
    parts = [cols] * 4 if kind == "four" else np.array_split(cols, d)
    brows = np.concatenate([np.full(len(p), 1 + k) for k, p in enumerate(parts)])
    bcols = np.concatenate(parts)
    arows, acols = np.array([0] * d + [5, 5]), np.array(list(range(1, d + 1)) + [n - 1, n - 2])
    return (_csr(n, arows, acols, rng.integers(1, 4, arows.size).astype(np.float32)),
            _csr(n, brows, bcols, rng.integers(1, 4, brows.size).astype(np.float32)))


@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("kind", ["once", "four", "chain", "run"])
def test_one_product_row_at_every_table_boundary(gpu, mode, monkeypatch, kind, c):
    set_knob(monkeypatch, "spgemm_wave_slots", WAVE_SLOTS)
    set_knob(monkeypatch, "spgemm_lds_slots", LDS_SLOTS)
    a, b = row_case(kind, c)
    for op in SEMIRINGS.values():
        got = _check(a, b, op, mode=mode, tables=(WAVE_SLOTS, LDS_SLOTS), what="%s c=%d" % (kind, c))
        assert got.adj_indptr[1] == c and got.nnz == c


@pytest.mark.parametrize("p", [65, 257, 1200])
def test_many_products_into_one_column(gpu, mode, monkeypatch, p):
    set_knob(monkeypatch, "spgemm_wave_slots", WAVE_SLOTS)
    set_knob(monkeypatch, "spgemm_lds_slots", LDS_SLOTS)
    n = 2048
    rng = np.random.default_rng(p)
    a = _csr(n, np.zeros(p, np.int64), 1 + np.arange(p), rng.integers(1, 4, p).astype(np.float32))
    b = _csr(n, 1 + np.arange(p), np.full(p, 777), rng.integers(1, 4, p).astype(np.float32))
    for op in SEMIRINGS.values():
        assert _check(a, b, op, mode=mode, tables=(WAVE_SLOTS, LDS_SLOTS), what="p=%d" % p).nnz == 1


@functools.lru_cache(maxsize=None)
def random_pair(values="int"):
    """n = 512, mean degree 8, four rows and four columns of degree 200"""
    n = 512
    rng = np.random.default_rng(11)
    out = []
    for seed in (21, 22):
        m = random_csr(n, 8 * n, seed, values)
        rows = np.repeat(np.arange(n), np.diff(m.adj_indptr.astype(np.int64)))
        heavy = rng.choice(n, 8, replace=False)
        hr = np.concatenate([np.full(200, r) for r in heavy[:4]] + [rng.choice(n, 200, replace=False) for _ in heavy[4:]])
        hc = np.concatenate([rng.choice(n, 200, replace=False) for _ in heavy[:4]] + [np.full(200, r) for r in heavy[4:]])
        key = np.unique(np.concatenate([rows * n + m.adj_indices, hr * n + hc]))
        data = rng.integers(1, 4, key.size) if values == "int" else rng.standard_normal(key.size)
        out.append(_csr(n, key // n, key % n, data.astype(np.float32)))
    return tuple(out)


@pytest.mark.parametrize("masking", sorted(MASKS))
@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
@pytest.mark.parametrize("pair", ["AA", "AB"])
def test_random_graph(gpu, mode, pair, semiring, masking):
    a, b = random_pair()
    use_mask, complement = MASKS[masking]
    _check(a, a if pair == "AA" else b, SEMIRINGS[semiring], a if use_mask else None, complement, mode, what=pair)


def test_signed_cancelling_reals_keep_their_entries(gpu, mode):
    a, b = (m.copy() for m in random_pair("real"))
    # row 0 of A = {1: x, 2: -x}; rows 1 and 2 of B hold column 9 with the same value: C[0, 9] cancels to 0.0 and stays
    n = a.num_rows
    keep = np.repeat(np.arange(n), np.diff(a.adj_indptr.astype(np.int64))) != 0
    rows = np.repeat(np.arange(n), np.diff(a.adj_indptr.astype(np.int64)))[keep]
    a = _csr(n, np.concatenate([rows, [0, 0]]), np.concatenate([a.adj_indices[keep], [1, 2]]), np.concatenate([a.adj_data[keep], [1.7, -1.7]]))
    brows = np.repeat(np.arange(n), np.diff(b.adj_indptr.astype(np.int64)))
    keep = ~(np.isin(brows, (1, 2)))
    b = _csr(n, np.concatenate([brows[keep], [1, 2, 2]]), np.concatenate([b.adj_indices[keep], [9, 9, 30]]), np.concatenate([b.adj_data[keep], [0.3, 0.3, 2.0]]))
    c = _check(a, b, M.kMulAdd, mode=mode, exact=False, what="cancelling")
    assert c.adj_indices[:c.adj_indptr[1]].tolist() == [9, 30] and c.adj_data[0] == 0.0
    _check(a, a, M.kMulAdd, a, True, mode, exact=False, what="real AA")


def test_refusals_and_empty_operands(gpu):
    a, b = random_pair()
    n = a.num_rows
    pa, va = _plan(a), _values(a)
    out = capi.DeviceBuffer.from_host(np.full(n + 1 + GUARD, G32, np.uint32))
    small = random_csr(64, 100, 1)
    shuffled = _csr_as_given(n, [3, 3, 3], [9, 4, 7])
    for bad, message in ((_plan(a, flags=0), "keeps no row copy"), (_plan(shuffled), "strictly ascending"), (_plan(small), "vertices"),
                         (_plan(a, 0, 256), "row shard")):
        for x, y, m in ((bad, pa, None), (pa, bad, None), (pa, pa, bad)):
            with pytest.raises(capi.GraphLilyError, match=message) as err:
                x.spgemm_symbolic(y, out, m)
            assert err.value.code == capi.GL_ERR_UNSUPPORTED
    with pytest.raises(capi.GraphLilyError) as err:
        pa.spgemm_symbolic(pa, out, None, complement=True)
    assert err.value.code == capi.GL_ERR_INVALID_ARG
    pa.spgemm_symbolic(pa, out)
    with pytest.raises(capi.GraphLilyError) as err:
        pa.spgemm_numeric(pa, M.kMulAdd, va, va, out, out, None)
    assert err.value.code == capi.GL_ERR_INVALID_ARG
    empty = io.CSRMatrix(n, n, np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(n + 1, np.uint32))
    for x, y, m in ((empty, a, None), (a, empty, None), (a, a, empty)):
        for op in SEMIRINGS.values():
            assert _check(x, y, op, m, what="empty").nnz == 0


def test_module_and_two_hop_driver(gpu):
    a, b = random_pair()
    m = M.SpGEMMModule()
    m.set_up_runtime()
    m.load_and_format_matrices(a, b)
    m.load_mask_matrix(a)
    m.send_matrices_host_to_device()
    for semiring in (M.ArithmeticSemiring, M.LogicalSemiring, M.TropicalSemiring):
        for mask_type, (use_mask, complement) in ((M.kNoMask, (False, False)), (M.kMaskWriteToOne, (True, False)), (M.kMaskWriteToZero, (True, True))):
            m.set_semiring(semiring)
            m.set_mask_type(mask_type)
            m.run()
            got, want = m.send_results_device_to_host(), spgemm_model(a, b, semiring.op, a if use_mask else None, complement)[0]
            assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in ("adj_indptr", "adj_indices", "adj_data"))
    th = app.TwoHop()
    th.load_and_format_matrix(a)
    th.send_matrix_host_to_device()
    g = th.graph_
    eye = io.CSRMatrix(g.num_rows, g.num_rows, np.ones(g.num_rows), np.arange(g.num_rows), np.arange(g.num_rows + 1))
    paths = th.run("paths")
    assert app.validate_spgemm(g, g, paths, M.kMulAdd, eye, True) == paths.nnz > 0
    cand = th.run("candidates")
    sim = app.Similarity()
    sim.load_and_format_matrix(a)
    for s in (0, 7, 300):
        assert cand.adj_indices[cand.adj_indptr[s]:cand.adj_indptr[s + 1]].tolist() == sim.two_hop_pairs([s])[:, 1].tolist()


def test_cpp_driver_on_the_golden_file(gpu, golden_dir, tmp_path):
    path = os.path.join(golden_dir, GOLDEN)
    a = io.load_csr_matrix_from_float_npz(path)
    r = subprocess.run([SPGEMM_DRIVER, path, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SpGEMM OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    th = app.TwoHop()
    th.load_and_format_matrix(path)
    th.send_matrix_host_to_device()
    want = {what: th.run(what) for what in ("paths", "candidates")}
    m = M.SpGEMMModule()
    m.set_up_runtime()
    m.load_and_format_matrices(a)
    m.load_mask_matrix(a)
    m.send_matrices_host_to_device()
    for semiring, sr in (("muladd", M.ArithmeticSemiring), ("andor", M.LogicalSemiring), ("addmin", M.TropicalSemiring)):
        for masking, mask_type in (("none", M.kNoMask), ("mask", M.kMaskWriteToOne), ("complement", M.kMaskWriteToZero)):
            m.set_semiring(sr)
            m.set_mask_type(mask_type)
            m.run()
            want["%s_%s" % (semiring, masking)] = m.send_results_device_to_host()
            model = spgemm_model(m.a_, m.a_, sr.op, m.a_ if mask_type != M.kNoMask else None, mask_type == M.kMaskWriteToZero)[0]
            assert np.array_equal(want["%s_%s" % (semiring, masking)].adj_data, model.adj_data)
    for name, c in want.items():
        assert c.nnz > 0 and "%s: nnz %d," % (name, c.nnz) in r.stdout, name
        for field, dtype in (("indptr", np.uint32), ("indices", np.uint32), ("val", np.float32)):
            got = np.fromfile(os.path.join(str(tmp_path), "cpp_%s_%s.bin" % (name, field)), dtype=dtype)
            assert np.array_equal(got, getattr(c, "adj_data" if field == "val" else "adj_" + field)), (name, field)

