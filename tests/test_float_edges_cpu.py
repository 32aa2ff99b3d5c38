"""The inputs and expectations of tests/test_gpu_float_edges.py, proven on the CPU oracle alone: every generator and matrix goes
through O.spmv / O.spmspv, which must meet the any-order f32 bound against arith_expected on every row with the same non-finite
classes, and the structural and share conditions the GPU tests rely on must hold (poisoned rows between 1 % and 50 %, non-zero
subnormal rows at least 25 %, cancelling rows that really cancel).  Needs no GPU."""
import numpy as np
import pytest

from oracle import oracle as O

from helpers import (EDGE_HOT, EDGE_HUBS, EDGE_KINDS, MASKS, SEMIRINGS, arith_expected, arith_expected_frontier, assert_arith_scatter,
                     assert_arith_signed, cancelling_csc, edge_matrix, edge_poison, frontier_of, logical_odd_inputs, mask_keep,
                     min_plus_inputs, rand01, rmat_signed, signed_inputs, stable_seed, to_oracle, wide_matrix, wide_poison)

MATRICES = [("edge", k) for k in EDGE_KINDS] + [("wide", "general"), ("wide", "pattern")]
KINDS = ["signed", "cancelling", "wide", "subnormal", "poison"]


def _matrix(which, layout):
    return edge_matrix(layout) if which == "edge" else wide_matrix()


def test_edge_matrix_structure():
    n = 4096
    m = {k: edge_matrix(k, n) for k in EDGE_KINDS}
    g = m["general"]
    for k in EDGE_KINDS:
        assert np.array_equal(m[k].adj_indptr, g.adj_indptr) and np.array_equal(m[k].adj_indices, g.adj_indices)
    lens = np.diff(g.adj_indptr.astype(np.int64))
    col = g.adj_indices[:g.nnz].astype(np.int64)
    row = np.repeat(np.arange(n), lens)
    deg = np.bincount(col, minlength=n)
    assert np.all(lens[::97] == 0) and np.all(lens[np.arange(n) % 97 != 0] > 0)
    assert all(lens[r] >= n // 2 for r in EDGE_HUBS) and np.sort(lens)[-4] < 32
    assert deg[n - 2] == 0 and 8 <= deg[n - 1] <= n // 2
    assert deg[:EDGE_HOT].min() > 5 * deg[EDGE_HOT:].max()                 # the 64 hot columns are the 64 of highest degree
    hot_per_row = np.bincount(row[col < EDGE_HOT], minlength=n)
    plain = np.array([r for r in range(EDGE_HOT, n) if r % 97 and r not in EDGE_HUBS])   # (below EDGE_HOT the diagonal is a hot column)
    assert np.array_equal(hot_per_row[plain], plain % 17)
    assert np.all(np.diff(col)[np.diff(row) == 0] > 0)                      # rows ascend, no duplicates
    diag = col == row
    assert diag.sum() > n // 4
    # pattern: constant columns; pattern_diag: constant apart from the diagonal, which always differs and is negative on half
    for k in ("pattern", "pattern_diag"):
        a = m[k].adj_data[:g.nnz]
        off = ~diag if k == "pattern_diag" else np.ones(g.nnz, bool)
        first = np.full(n, np.nan, np.float32)
        first[col[off][::-1]] = a[off][::-1]
        assert np.array_equal(a[off].view(np.uint32), first[col[off]].view(np.uint32))
        if k == "pattern_diag":
            has = deg - np.bincount(col[diag], minlength=n) > 0
            d = np.flatnonzero(diag)
            assert np.all(a[d][has[col[d]]] != first[col[d]][has[col[d]]])
            assert 0.4 < (a[d] < 0).mean() < 0.6
    a = g.adj_data[:g.nnz]
    assert (a < 0).any() and (a > 0).any() and np.unique(a).size > g.nnz // 2


def test_wide_matrix_structure():
    m = wide_matrix()
    assert (m.num_rows, m.num_cols, m.nnz) == (1024, 262144, 4096)
    # 16 row blocks of 64 rows: the sorted columns of a block are mostly further apart than the 255 an 8-bit delta spans
    col = m.adj_indices.astype(np.int64).reshape(16, -1)
    gaps = np.diff(np.sort(col, axis=1), axis=1)
    assert (gaps > 255).mean() > 0.6


def _case(which, layout, kind):
    m = _matrix(which, layout)
    poison = None
    if kind == "poison":
        poison = (lambda a: edge_poison(m, layout, a)) if which == "edge" else (lambda a: wide_poison(m, a))
    m.adj_data, x = signed_inputs(np.random.default_rng(stable_seed(which, layout, kind)), m, kind, layout=layout, poison=poison)
    return m, x


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which,layout", MATRICES)
def test_oracle_meets_the_bounds_spmv(which, layout, kind):
    if kind == "cancelling" and layout != "general":
        with pytest.raises(AssertionError):
            _case(which, layout, kind)
        return
    m, x = _case(which, layout, kind)
    exact, abs_sum, lens = arith_expected(m, x)
    mask = rand01(m.num_rows, 7)
    for mk in MASKS:
        ref = O.spmv(to_oracle(m), x, O.MULADD, 0.0, mask, MASKS[mk]) if MASKS[mk] else O.spmv(to_oracle(m), x, O.MULADD, 0.0)
        assert_arith_scatter(ref, exact, abs_sum, lens, mask_keep(mk, mask), "%s %s %s %s" % (which, layout, kind, mk))
    # the sharper bound is met by the correctly rounded f64 sum, and NOT by a result that is off by two f32 roundings
    good = exact.astype(np.float32)
    assert_arith_signed(good, exact, abs_sum, lens, False)
    fin = np.isfinite(exact) & (np.abs(exact) > 2.0 ** -100)
    if fin.any():
        wrong = good.copy()
        wrong[fin] = wrong[fin] * np.float32(1 + 2.0 ** -22)
        if kind != "cancelling":          # (where rows cancel, abs_sum dwarfs the result and the split term allows it)
            with pytest.raises(AssertionError):
                assert_arith_signed(wrong, exact, abs_sum, lens, True)
    rows = m.num_rows
    if kind == "subnormal":
        e32 = exact.astype(np.float32)
        assert ((e32 != 0) & (np.abs(e32) < np.float32(2.0 ** -126))).sum() >= rows // 4
        p = np.abs(m.adj_data[:m.nnz].astype(np.float64) * x.astype(np.float64)[m.adj_indices[:m.nnz]])
        assert p.max() < 2.0 ** -126          # every product is subnormal
    if kind == "cancelling":
        even = (lens > 0) & (lens % 2 == 0)
        assert even.sum() > rows // 4
        assert (np.abs(exact[even]) <= 1e-5 * abs_sum[even]).mean() >= 0.5
    if kind == "wide":
        with np.errstate(all="ignore"):
            p = np.abs(m.adj_data[:m.nnz].astype(np.float64) * x.astype(np.float64)[m.adj_indices[:m.nnz]])
        assert p.max() > 1e20 and p.min() < 1e-20 and np.all(np.isfinite(exact.astype(np.float32)))
    if kind == "poison":
        bad = ~np.isfinite(exact)
        assert 0.01 * rows <= bad.sum() <= 0.5 * rows
        with np.errstate(all="ignore"):
            p = m.adj_data[:m.nnz] * x[m.adj_indices[:m.nnz]]
        row = np.repeat(np.arange(rows), lens)
        nan_product = np.bincount(row, weights=np.isnan(p), minlength=rows) > 0
        assert (np.isnan(exact) & ~nan_product).any(), "no row expects NaN from inf - inf"
        assert (exact == np.inf).any() and (exact == -np.inf).any() and nan_product.any()
        touched = np.bincount(row, weights=~np.isfinite(x[m.adj_indices[:m.nnz]]), minlength=rows) > 0
        assert np.array_equal(bad, touched)                          # non-finite exactly in the rows that hold a poisoned column
        if which == "edge":
            n = m.num_cols
            assert np.isnan(x[n - 2]) and np.isinf(x[n - 1]) and np.isinf(x[3]) and any(bad[r] for r in EDGE_HUBS)


@pytest.mark.parametrize("sem", ["Tropical", "TropicalFloatInf"])
@pytest.mark.parametrize("which,layout", [("edge", k) for k in EDGE_KINDS] + [("wide", "general")])
def test_min_plus_inputs(which, layout, sem):
    op, zero = SEMIRINGS[sem]
    m = _matrix(which, layout)
    m.adj_data, x = min_plus_inputs(np.random.default_rng(stable_seed(which, layout, sem)), m, zero, layout)
    a = m.adj_data[:m.nnz]
    assert np.all(np.isfinite(a)) and a.min() == -8 and a.max() >= 8 and np.all(a * 8 == np.round(a * 8))
    assert (a.view(np.uint32) == 0x80000000).any() and (a.view(np.uint32) == 0).any()
    assert (x == np.inf).any() and (x == -np.inf).any() and 0.4 < (x == np.float32(zero)).mean() < 0.6
    ref = O.spmv(to_oracle(m), x, op, zero)
    assert not np.isnan(ref).any() and (ref == -np.inf).any() and (ref < 0).any() and (ref == np.float32(zero)).any()
    # value for value what a float64 evaluation of min(zero, min_i a_i + x_i) gives (the sums of eighths and f32 are one rounding)
    row = np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64)))
    t = (a + x[m.adj_indices[:m.nnz]]).astype(np.float64)
    want = np.full(m.num_rows, float(zero))
    np.minimum.at(want, row, t)
    assert np.array_equal(ref, want.astype(np.float32))


@pytest.mark.parametrize("layout", ["general", "pattern"])
def test_logical_odd_inputs(layout):
    m = edge_matrix(layout)
    m.adj_data, x, mask = logical_odd_inputs(np.random.default_rng(stable_seed("odd", layout)), m, layout)
    a = m.adj_data[:m.nnz]
    for arr in (a, x, mask):
        assert np.isnan(arr).any() and np.isinf(arr).any() and (arr.view(np.uint32) == 0x80000000).any()
        assert ((arr != 0) & (np.abs(arr) < np.float32(2.0 ** -126))).any()
    ref = O.spmv(to_oracle(m), x, O.ANDOR, 0.0)
    col = m.adj_indices[:m.nnz].astype(np.int64)
    row = np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64)))
    want = np.bincount(row, weights=(a != 0) & (x[col] != 0), minlength=m.num_rows) > 0       # NaN != 0, a subnormal != 0
    assert np.array_equal(ref, want.astype(np.float32)) and 0.2 < want.mean() < 0.999
    if layout == "pattern":
        nan_cols = np.unique(col[np.isnan(a)])
        assert nan_cols.size > 50 and np.unique(a[np.isnan(a)].view(np.uint32)).size == 1


def test_cancelling_csc_and_the_oracle():
    csc, v1, v2, ra, rb, q = cancelling_csc()
    assert csc.num_rows == 4096 and np.all(np.diff(csc.adj_indptr.astype(np.int64)) == 4) and int(v1["index"][0]) == 256
    oc = to_oracle(csc)
    for v, first in ((v1, True), (v2, False)):
        exact, abs_sum, lens = arith_expected_frontier(csc, v)
        ref = O.spmspv(oc, v, O.MULADD, 0.0)
        assert_arith_scatter(ref, exact, abs_sum, lens, None)
        assert np.all(lens[ra] == 2) and np.all(lens[rb] == 3) and np.all(abs_sum[ra] > 0)
        if first:
            assert np.all(exact[ra] == 0) and np.all(ref[ra] == 0) and np.array_equal(ref[rb], q) and np.all(q != 0)
        else:
            assert np.all(ref[ra] != 0) and np.all(ref[rb] != q)
        assert (exact != 0).sum() > 500


@pytest.mark.parametrize("layout", ["general", "pattern"])
@pytest.mark.parametrize("kind", ["signed", "wide"])
def test_rmat_signed_and_the_oracle(kind, layout):
    csr, csc, x = rmat_signed(kind, layout)
    rng = np.random.default_rng(3)
    for density in (0.0005, 0.25):
        v = frontier_of(x, np.flatnonzero(rng.random(csc.num_cols) < density))
        exact, abs_sum, lens = arith_expected_frontier(csc, v)
        assert_arith_scatter(O.spmspv(to_oracle(csc), v, O.MULADD, 0.0), exact, abs_sum, lens, None, "%s %s %g" % (kind, layout, density))
        assert (exact < 0).any() and (exact > 0).any()
    # the frontier-restricted expectation is the dense one when the frontier is every column
    full = frontier_of(x, np.arange(csc.num_cols))
    e1, s1, l1 = arith_expected_frontier(csc, full)
    e2, s2, l2 = arith_expected(csr, x)
    assert np.array_equal(l1, l2) and np.allclose(e1, e2, rtol=1e-12, atol=0) and np.allclose(s1, s2, rtol=1e-12, atol=0)
