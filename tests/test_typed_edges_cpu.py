"""The inputs and expectations of tests/test_gpu_typed_edges.py, proven on the CPU alone: on every matrix, layout, value type,
semiring, kind and zero used there the oracle's integer restatement (O.spmv_words / O.spmspv_words) equals helpers.words_expected,
a second restatement written from the ALUs with numpy uint64, word for word; and the shares the GPU tests rely on hold -- saturated
next to unsaturated rows, a hub row whose sum crosses 2^32 only across its column-contiguous halves, rows at and below the
(min,+) zero, both outcomes of (||,&&), the SpMSpV vectors whose doubling saturates.  Needs no GPU."""
import numpy as np
import pytest

from oracle import oracle as O

from helpers import (CONTENDED_N, CONTENDED_ROWS, EDGE_KINDS, HUB_CROSSING_ROW, HUB_CROSSING_WORD, HUB_SMALL_ROW, MASKS, VALUE_TYPES,
                     VAL_UFIXED, WORD_MAX, WORD_OPS, contended_case, contended_csc, edge_matrix, frontier_case, long_columns_case,
                     random_csc, rmat_csc, rmat_sssp_csc, spmv_words_reference, stable_seed, typed_inputs, wide_matrix, word_nonzero_zero, word_one, word_vec,
                     word_zero, words_expected, words_expected_frontier, words_mask_spmspv, words_mask_spmv)

MATRICES = [("edge", k) for k in EDGE_KINDS] + [("wide", "general"), ("wide", "pattern")]


def _matrix(which, layout):
    return edge_matrix(layout) if which == "edge" else wide_matrix()


def _kinds(op):
    return ("small", "large") if op == 0 else (None,)


def test_the_restatement_on_known_words():
    """The corners of the three ALUs, by hand: AP_RND rounds half up, AP_SAT clamps the product and the sum, unsigned wraps."""
    ip, ix = np.array([0, 2, 3, 5, 5], np.uint32), np.array([0, 1, 2, 3, 4], np.uint32)
    a = np.array([1, 3, 0xffffffff, 192 << 24, 64 << 24], np.uint32)
    x = np.array([1 << 23, (1 << 23) - 1, 200 << 24, 1 << 24, 1 << 24], np.uint32)
    f, u = VAL_UFIXED, VALUE_TYPES["unsigned"]
    assert words_expected(ip, ix, a, x, 0, f, 0).tolist() == [2, 0xffffffff, 0xffffffff, 0]      # 1 + 1; a product, then a sum that clamps
    assert words_expected(ip, ix, a, x, 0, f, 5).tolist() == [7, 0xffffffff, 0xffffffff, 5]
    assert words_expected(ip, ix, a, x, 0, u, 0).tolist() == [(1 << 23) + 3 * ((1 << 23) - 1), (0xffffffff * (200 << 24)) & WORD_MAX, 0, 0]
    assert words_expected(ip, ix, a, x, 1, f, 0).tolist() == [1 << 24, 1 << 24, 1 << 24, 0]
    assert words_expected(ip, ix, a, x, 1, u, 2).tolist() == [1, 1, 1, 2]                          # nothing applied: `zero` itself
    assert words_expected(ip, ix, a, x, 2, f, 255 << 24).tolist() == [1 + (1 << 23), 255 << 24, 65 << 24, 255 << 24]
    assert words_expected(ip, ix, a, x, 2, f, WORD_MAX).tolist() == [1 + (1 << 23), WORD_MAX, 65 << 24, WORD_MAX]      # a sum that clamps
    assert words_expected(ip, ix, a, x, 2, u, WORD_MAX).tolist() == [1 + (1 << 23), (200 << 24) - 1, 65 << 24, WORD_MAX]     # wraps
    for op in (0, 1, 2):
        for vt in (f, u):
            assert np.array_equal(words_expected(ip, ix, a, x, op, vt, 3), O.spmv_words(ip, ix, a, x, op, vt, 3))


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
@pytest.mark.parametrize("which,layout", MATRICES)
def test_oracle_equals_the_restatement_spmv(which, layout, vt_name):
    vt = VALUE_TYPES[vt_name]
    m = _matrix(which, layout)
    ip, ix, rows = m.adj_indptr, m.adj_indices, m.num_rows
    lens = np.diff(ip.astype(np.int64))
    for op in WORD_OPS.values():
        for kind in _kinds(op):
            what = "%s %s %s op %d %s" % (which, layout, vt_name, op, kind)
            a, x, mask, zero = typed_inputs(np.random.default_rng(stable_seed(which, layout, vt_name, op, kind)), m, layout, vt, op, kind)
            assert zero == word_zero(vt, op) and set(np.unique(mask).tolist()) == {0, 1, 0x80000000}
            for arr in (a, x):
                assert (arr == 0).mean() > 0.02
                if not (op == 0 and kind == "small" and arr is x):
                    assert (arr == 0x80000000).mean() > 0.005
            if layout != "general":                                      # column-constant apart from a differing diagonal
                col = ix[:m.nnz].astype(np.int64)
                row = np.repeat(np.arange(rows), lens)
                off = col != row if layout == "pattern_diag" else np.ones(m.nnz, bool)
                first = np.zeros(m.num_cols, np.uint32)
                first[col[off][::-1]] = a[off][::-1]
                assert np.array_equal(a[off], first[col[off]])
                if layout == "pattern_diag":
                    d = np.flatnonzero(~off)
                    has = np.bincount(col[off], minlength=m.num_cols) > 0
                    assert len(d) > rows // 4 and np.all(a[d][has[col[d]]] != first[col[d]][has[col[d]]])
            ref = O.spmv_words(ip, ix, a, x, op, vt, zero)
            assert np.array_equal(ref, words_expected(ip, ix, a, x, op, vt, zero)), what
            for mk, mt in MASKS.items():
                assert np.array_equal(O.spmv_words(ip, ix, a, x, op, vt, zero, mask if mt else None, mt), words_mask_spmv(ref, mask, mt)), (what, mk)
            nz = word_nonzero_zero(vt, op, ref)
            ref_nz = O.spmv_words(ip, ix, a, x, op, vt, nz)
            assert nz != zero and np.array_equal(ref_nz, words_expected(ip, ix, a, x, op, vt, nz)), what
            sat, live = ref == WORD_MAX, (ref != 0) & (ref != WORD_MAX)
            if op == 0 and kind == "small":
                assert not sat.any() and len(np.unique(ref)) >= (4000 if which == "edge" else 900), what
            if op == 0 and kind == "large" and vt == VAL_UFIXED:
                share = 0.25 if which == "edge" else 0.1
                assert sat.sum() >= share * rows and live.sum() >= share * rows, (what, int(sat.sum()), int(live.sum()))
                if which == "edge" and layout == "general":
                    assert lens[HUB_SMALL_ROW] >= rows // 2 and live[HUB_SMALL_ROW] and sat[HUB_CROSSING_ROW]
                    lo, hi = int(ip[HUB_CROSSING_ROW]), int(ip[HUB_CROSSING_ROW + 1])
                    assert np.all(a[lo:hi] == HUB_CROSSING_WORD)
                    p = (a[lo:hi].astype(np.uint64) * x[ix[lo:hi].astype(np.int64)].astype(np.uint64) + np.uint64(1 << 23)) >> np.uint64(24)
                    c = np.concatenate([[0], np.cumsum(p)])
                    half = (hi - lo) // 2
                    assert c[-1] > 1.25 * 2.0 ** 32                       # the exact sum is well past the clamp ...
                    assert (c[half:] - c[:len(c) - half]).max() < WORD_MAX    # ... and no column-contiguous half of the row reaches it
            if op == 0 and vt != VAL_UFIXED:
                assert len(np.unique(ref)) > 0.9 * (lens > 0).sum(), what     # modular sums: every row its own word
            if op == 0:
                assert (ref_nz != ref)[~sat].mean() > 0.9, what          # (a saturated row stays saturated)
            if op == 1:
                assert min((ref == 0).sum(), (ref == word_one(vt)).sum()) >= 40, what
                assert (lens == 0).sum() == (43 if which == "edge" else 0)
                # zero = 2: the reference's loop leaves 2 in exactly the rows without stored entries, every other row is ONE; the
                # library's y = zero (+) sum gives ONE there too (spmv_words_reference) -- the only rows on which the two differ
                assert set(np.unique(ref_nz).tolist()) <= {2, word_one(vt)} and ((ref_nz == 2) == (lens == 0)).all()
                for mk, mt in MASKS.items():
                    want = spmv_words_reference(m, a, x, op, vt, nz, mask, mt)
                    plain = O.spmv_words(ip, ix, a, x, op, vt, nz, mask if mt else None, mt)
                    assert np.array_equal(want[lens > 0], plain[lens > 0]) and set(want[lens == 0].tolist()) <= {0, word_one(vt)}
                    assert np.array_equal(spmv_words_reference(m, a, x, op, vt, zero, mask, mt), O.spmv_words(ip, ix, a, x, op, vt, zero, mask if mt else None, mt))
            if op == 2:
                assert (ref < zero).any(), what
                if vt == VAL_UFIXED or (lens == 0).any():                # (unsigned: a + 0xffffffff wraps to a - 1, only an empty row stays at zero)
                    assert (ref == zero).any(), what
                assert 0.25 * rows <= (ref_nz == nz).sum() <= 0.75 * rows, (what, int((ref_nz == nz).sum()))
                if vt == VAL_UFIXED:                                     # a row whose every product saturates: 0xffffffff before the final min
                    assert (words_expected(ip, ix, a, x, op, vt, WORD_MAX)[lens > 0] == WORD_MAX).any(), what


def _check_frontier(csc, data, v, mask, zero, op, vt, what):
    """oracle == restatement for the vector, unmasked and under both masks -> the unmasked result."""
    n = csc.num_rows
    ref = O.spmspv_words(csc.adj_indptr, csc.adj_indices, data, v, n, op, vt, zero)
    assert np.array_equal(ref, words_expected_frontier(csc.adj_indptr, csc.adj_indices, data, v, n, op, vt, zero)), what
    for mk, mt in MASKS.items():
        got = O.spmspv_words(csc.adj_indptr, csc.adj_indices, data, v, n, op, vt, zero, mask if mt else None, mt)
        assert np.array_equal(got, words_mask_spmspv(ref, mask, mt, zero)), (what, mk)
    return ref


def _mask_is_mixed(mask, zero):
    return all((mask == w).mean() > 0.2 for w in (zero, 7, 0x80000000))


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_spmspv_long_columns_inputs(vt_name):
    vt = VALUE_TYPES[vt_name]
    for op in WORD_OPS.values():
        csc, data, vs, mask, zero = long_columns_case(vt_name, op)
        n = csc.num_rows
        deg = np.diff(csc.adj_indptr.astype(np.int64))
        assert n == 16384 and (deg > 0).sum() == 24 and deg[deg > 0].min() == 4097 and deg.max() < 8192
        assert int(vs[0]["index"][0]) == 24 and int(vs[1]["index"][0]) == 48 and _mask_is_mixed(mask, zero)
        assert np.array_equal(np.sort(vs[1]["index"][1:25]), np.sort(vs[1]["index"][25:]))        # every column twice
        single, doubled = (_check_frontier(csc, data, v, mask, zero, op, vt, "long columns %s op %d" % (vt_name, op)) for v in vs[:2])
        assert (single != zero).sum() > n // 4
        if op == 0 and vt == VAL_UFIXED:
            sat, live = doubled == WORD_MAX, (doubled != 0) & (doubled != WORD_MAX)
            assert sat.sum() >= n // 10 and live.sum() >= n // 10
            assert ((single != WORD_MAX) & sat).sum() >= n // 20          # the clamp acts on bin + spilled accumulator together
        if op == 0 and vt != VAL_UFIXED:
            assert (doubled != single).mean() > 0.9


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_spmspv_contended_inputs(vt_name):
    vt = VALUE_TYPES[vt_name]
    csc = contended_csc()
    assert csc.num_rows == CONTENDED_N == 2049 * 64
    deg = np.diff(csc.adj_indptr.astype(np.int64))
    assert 5 <= deg.min() and deg.max() <= 8 and (deg >= 6).mean() > 0.99
    for r in CONTENDED_ROWS:
        assert np.array_equal(np.flatnonzero(np.bincount(np.repeat(np.arange(csc.num_cols), deg)[csc.adj_indices == r], minlength=csc.num_cols)),
                              np.arange(0, csc.num_cols, 4))
    for op in WORD_OPS.values():
        c, data, vs, mask, zero = contended_case(vt_name, op)
        assert [int(v["index"][0]) for v in vs] == [300, 5000] and _mask_is_mixed(mask, zero)
        for v in vs:
            ref = _check_frontier(c, data, v, mask, zero, op, vt, "contended %s op %d" % (vt_name, op))
            hits = (v["index"][1:] % 4 == 0).sum()
            assert hits >= 50 and (ref != zero).sum() > 1000
            if op == 0 and vt == VAL_UFIXED:
                assert ref[0] == WORD_MAX and 0 < ref[1] < WORD_MAX // 16


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_spmspv_other_inputs(vt_name):
    vt = VALUE_TYPES[vt_name]
    tiles = random_csc(40000, 6, 5, (3, 5000))
    assert np.sort(np.diff(tiles.adj_indptr.astype(np.int64)))[-3] >= 5000
    cut = rmat_sssp_csc()
    assert int(np.diff(cut.adj_indptr.astype(np.int64)).max()) <= 12288      # (else the default would not cut by entries)
    for op in WORD_OPS.values():
        for name, csc, counts in (("tiles", tiles, (300, 3000, 40000 // 3)), ("cuts", cut, (4097, 9000)), ("shards", rmat_csc(), (1000,))):
            data, vs, mask, zero = frontier_case(csc, name, vt_name, op, counts)
            assert _mask_is_mixed(mask, zero)
            for v in vs:
                ref = _check_frontier(csc, data, v, mask, zero, op, vt, "%s %s op %d" % (name, vt_name, op))
                assert (ref != zero).sum() > 100
        empty = word_vec([], [])
        ref = O.spmspv_words(cut.adj_indptr, cut.adj_indices, data, empty, cut.num_rows, op, vt, zero)
        assert np.all(ref == zero) and np.array_equal(ref, words_expected_frontier(cut.adj_indptr, cut.adj_indices, data, empty, cut.num_rows, op, vt, zero))
