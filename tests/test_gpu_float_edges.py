"""GPU parity of the float SpMV / SpMSpV paths on inputs the other files never use: signed and cancelling products, magnitudes
from 1e-30 to 1e30, subnormal products, inf / NaN in x and in the weights.  The matrices (helpers.edge_matrix, wide_matrix) reach
every structure of the general and pattern layouts -- hot table, row-packed records, hub rows, empty rows and columns, the
diagonal exceptions, the bridging dummies of the cold stream --, and every test asserts the structure it relies on.  The (+,x)
bounds are derived (helpers.assert_arith_signed / assert_arith_scatter), the other semirings are bit-exact.  The inputs and
expectations themselves are proven on the CPU oracle in tests/test_float_edges_cpu.py."""
import functools

import numpy as np
import pytest

from graphlily_amd import capi, io, module as M
from oracle import oracle as O

from helpers import (EDGE_KINDS, MASKS, SEMIRINGS, arith_expected, arith_expected_frontier, assert_arith_scatter,
                     assert_arith_signed, cancelling_csc, checked_sparse_result, edge_matrix, edge_poison, frontier_of,
                     logical_odd_inputs, mask_keep, min_plus_inputs, plan_formatters, rand01, rmat_signed, set_knob, signed_inputs, spmv_plans,
                     stable_seed, to_oracle, wide_matrix, wide_poison)

pytestmark = pytest.mark.gpu

FORMATTERS = plan_formatters()
EDGE = [("edge", k) for k in EDGE_KINDS]


@functools.lru_cache(maxsize=None)
def _structure(which, layout):
    return edge_matrix(layout) if which == "edge" else wide_matrix()


def _with_values(which, layout, data):
    m = _structure(which, layout).copy()
    m.adj_data = data
    return m


_plans = spmv_plans      # one plan per formatter flag, the structure asserted, the formatters' arrays compared (helpers.py)


def _run_plan(p, x, mask, rows, op, zero, mask_name):
    dx, dy = capi.DeviceBuffer.from_host(x), capi.DeviceBuffer(4 * rows)
    dm = capi.DeviceBuffer.from_host(mask) if MASKS[mask_name] else None
    p.run(dx, dm, dy, op, zero, MASKS[mask_name])
    return dy.read(np.float32, rows)


def _oracle_spmv(m, x, op, zero, mask_name, mask):
    if MASKS[mask_name] == O.NOMASK:
        return O.spmv(to_oracle(m), x, op, zero)
    return O.spmv(to_oracle(m), x, op, zero, mask, MASKS[mask_name])


# ------------------------------------------------------------------ (+,x) SpMV
@functools.lru_cache(maxsize=None)
def _arith_case(which, layout, kind):
    """The inputs of one (+,x) case, its expectation and the oracle's result per mask, computed once."""
    m = _structure(which, layout).copy()
    poison = None
    if kind == "poison":
        poison = (lambda a: edge_poison(m, layout, a)) if which == "edge" else (lambda a: wide_poison(m, a))
    m.adj_data, x = signed_inputs(np.random.default_rng(stable_seed(which, layout, kind)), m, kind, layout=layout, poison=poison)
    mask = rand01(m.num_rows, 7)
    oracle = {mk: _oracle_spmv(m, x, O.MULADD, 0.0, mk, mask) for mk in MASKS}
    return m, x, mask, arith_expected(m, x), oracle


def _check_arith(got, case, split, mask_name, what):
    m, x, mask, (exact, abs_sum, lens), oracle = case
    keep = mask_keep(mask_name, mask)
    assert_arith_signed(got, exact, abs_sum, lens, split, keep, what)
    assert_arith_scatter(got, oracle[mask_name].astype(np.float64), abs_sum, lens, keep, what + " vs oracle")


ARITH = [(w, l, k) for (w, l) in EDGE + [("wide", "general"), ("wide", "pattern")] for k in ("signed", "cancelling", "wide", "subnormal")
         if k != "cancelling" or l == "general"]


@pytest.mark.parametrize("shape", ["unsplit", "split"])
@pytest.mark.parametrize("which,layout,kind", ARITH)
def test_arith_signed(gpu, monkeypatch, which, layout, kind, shape):
    """A (+,x) row is one f32 rounding -- two on split plans -- away from the f64 sum of its f32 products: signed, cancelling
    (the exact result is ~1e-6 of the sum of magnitudes), 1e-30 .. 1e30 and subnormal products, on both formatters' plans."""
    case = _arith_case(which, layout, kind)
    m, x, mask, (exact, _, _), _ = case
    if kind == "subnormal":
        e32 = exact.astype(np.float32)
        assert ((e32 != 0) & (np.abs(e32) < np.float32(2.0 ** -126))).sum() >= m.num_rows // 4
    plans, split = _plans(monkeypatch, which, layout, shape, m)
    for p, fmt in zip(plans, ("host", "device")):
        for mk in ("NoMask", "WriteToZero"):
            got = _run_plan(p, x, mask, m.num_rows, O.MULADD, 0.0, mk)
            _check_arith(got, case, split, mk, "%s %s %s %s %s %s" % (which, layout, kind, shape, fmt, mk))


@pytest.mark.parametrize("shape", ["unsplit", "split"])
@pytest.mark.parametrize("which,layout", EDGE + [("wide", "general")])
def test_arith_poison_stays_in_its_rows(gpu, monkeypatch, which, layout, shape):
    """+inf, -inf and NaN in x -- in a hot column, a cold one, an empty one, the last one, one of a hub row, one whose diagonal
    is an exception -- make exactly the rows that hold such a column non-finite (NaN where inf meets -inf); every other row
    stays within the finite bound: no padding slot, bridging dummy, identity slot or private hub slot multiplies one of them
    into a row it does not belong to.  Every mask; unsplit also without / with the packed gather vector and with each helper."""
    case = _arith_case(which, layout, "poison")
    m, x, mask, (exact, _, _), _ = case
    bad = ~np.isfinite(exact)
    assert 0.01 * m.num_rows <= bad.sum() <= 0.5 * m.num_rows and np.isnan(exact).any() and np.isinf(exact).any()
    variants = [(None, None)]
    if shape == "unsplit":
        variants += [("spmv_compact", 0), ("spmv_compact", 1), ("spmv_helper", 0), ("spmv_helper", 1), ("spmv_helper", 2)]
    for knob, value in variants:
        if knob:
            set_knob(monkeypatch, knob, value)
        plans, split = _plans(monkeypatch, which, layout, shape, m, flags=FORMATTERS if knob is None else (0,))
        if knob:
            set_knob(monkeypatch, knob, None)
        for p in plans:
            for mk in MASKS:
                got = _run_plan(p, x, mask, m.num_rows, O.MULADD, 0.0, mk)
                _check_arith(got, case, split, mk, "poison %s %s %s %s=%s %s" % (which, layout, shape, knob, value, mk))


# ------------------------------------------------------------------ (min,+) SpMV
@pytest.mark.parametrize("shape", ["unsplit", "split"])
@pytest.mark.parametrize("which,layout", EDGE + [("wide", "general")])
@pytest.mark.parametrize("sem", ["Tropical", "TropicalFloatInf"])
def test_min_plus_signed(gpu, monkeypatch, sem, which, layout, shape):
    """(min,+) with negative weights and sums (the unsigned-max branch of the integer float min), -0.0 / 0.0, x = zero on half
    of the columns, +inf and -inf in x: value for value the oracle's.  (NaN is out of scope for (min,+))"""
    op, zero = SEMIRINGS[sem]
    data, x = min_plus_inputs(np.random.default_rng(stable_seed(which, layout, sem)), _structure(which, layout), zero, layout)
    m = _with_values(which, layout, data)
    mask = rand01(m.num_rows, 9)
    plans, _ = _plans(monkeypatch, which, layout, shape, m)
    for mk in MASKS:
        ref = _oracle_spmv(m, x, op, zero, mk, mask)
        assert (ref < 0).any() and (ref == -np.inf).any()
        for p in plans:
            got = _run_plan(p, x, mask, m.num_rows, op, zero, mk)
            if not np.array_equal(got, ref):
                i = np.flatnonzero(got != ref)
                raise AssertionError("%s %s %s %s %s: %d rows differ, first %d: got %r want %r" %
                                     (sem, which, layout, shape, mk, i.size, i[0], got[i[0]], ref[i[0]]))


# ------------------------------------------------------------------ (||,&&) SpMV on the value layouts
@pytest.mark.parametrize("shape", ["unsplit", "split"])
@pytest.mark.parametrize("layout", ["general", "pattern"])
def test_logical_odd_values_on_the_value_layouts(gpu, monkeypatch, layout, shape):
    """a && b on floats with explicit zeros, -0.0, NaN, negatives, +-inf and a subnormal in the weights, in x and in the mask,
    on the general layout (GL_PLAN_KEEP_VALUES) and the pattern layout (column-constant odd values: a column of bitwise-equal
    NaNs keeps the layout): bit-exact against the oracle and equal to the GL_PLAN_BOOLEAN plan's result."""
    s = _structure("edge", layout)
    data, x, mask = logical_odd_inputs(np.random.default_rng(stable_seed("odd", layout)), s, layout)
    m = _with_values("edge", layout, data)
    plans, _ = _plans(monkeypatch, "edge", layout, shape, m, extra=capi.GL_PLAN_KEEP_VALUES if layout == "general" else 0)
    boolean = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, flags=capi.GL_PLAN_BOOLEAN)
    assert boolean.info()["layout"] == "boolean"
    for mk in MASKS:
        ref = _oracle_spmv(m, x, O.ANDOR, 0.0, mk, mask)
        assert min((ref == 0).sum(), (ref == 1).sum()) > 200
        for p in plans + [boolean]:
            got = _run_plan(p, x, mask, m.num_rows, O.ANDOR, 0.0, mk)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (layout, shape, mk, p.info()["layout"])


# ------------------------------------------------------------------ the reference-order layout
@pytest.mark.parametrize("kind", ["signed", "wide", "subnormal", "poison"])
def test_reference_order_signed(gpu, kind):
    """GL_PLAN_REFERENCE_ORDER evaluates the oracle's own loop: word for word its results on signed, wide, subnormal and
    poisoned inputs, for (+,x) and (min,+); on NaN rows only NaN-ness is compared (the default NaN of x86 and of the GPU are
    different words)."""
    m, x, mask, _, _ = _arith_case("edge", "general", kind)
    plan = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, flags=capi.GL_PLAN_REFERENCE_ORDER)
    assert plan.info()["layout"] == "reference-order" and plan.info()["finite_values"]
    for sem in ("Arithmetic", "Tropical", "TropicalFloatInf"):
        op, zero = SEMIRINGS[sem]
        for mk in ("NoMask", "WriteToZero"):
            ref = _oracle_spmv(m, x, op, zero, mk, mask)
            got = _run_plan(plan, x, mask, m.num_rows, op, zero, mk)
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan), (kind, sem, mk)
            assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]), (kind, sem, mk)
            if kind == "poison" and op == 0 and mk == "NoMask":
                assert nan.any() and np.isinf(ref).any()


# ------------------------------------------------------------------ SpMSpV
def _spmspv_module(csc, mask, pull=False):
    mod = M.SpMSpVModule(512)
    mod.set_semiring(M.ArithmeticSemiring)
    mod.set_mask_type(M.kNoMask)
    mod.set_up_runtime()
    mod.load_and_format_matrix(csc)
    mod.send_matrix_host_to_device()
    if pull:
        mod.enable_own_pull()
    mod.send_mask_host_to_device(mask)
    return mod


def _spmspv_run(mod, csc, v, mask_name, mask, what):
    """One run, the list's form checked, the densified result against the frontier-restricted expectation and the oracle."""
    mod.set_mask_type(MASKS[mask_name])
    mod.send_vector_host_to_device(v)
    mod.run()
    got = checked_sparse_result(mod, 0.0, csc.num_rows)
    exact, abs_sum, lens = arith_expected_frontier(csc, v)
    keep = mask_keep(mask_name, mask)
    assert_arith_scatter(got, exact, abs_sum, lens, keep, what)
    ref = O.spmspv(to_oracle(csc), v, O.MULADD, 0.0, mask, MASKS[mask_name])
    assert_arith_scatter(got, ref.astype(np.float64), abs_sum, lens, keep, what + " vs oracle")
    return got


@pytest.mark.parametrize("mask_name", list(MASKS))
def test_tiny_run_cancels_and_comes_back(gpu, monkeypatch, mask_name):
    """The one-workgroup kernel takes "the old value was the fill value" for "first product to reach this row".  Rows whose
    products cancel exactly are left at the fill value and not emitted; rows that return to it and are reached again are
    appended twice and must come out once, with the third product; a second vector over the same columns that does not cancel
    sees nothing of the first run, and the first vector again nothing of the second."""
    set_knob(monkeypatch, "spmspv_tiny", "1")
    csc, v1, v2, ra, rb, q = cancelling_csc()
    mask = rand01(csc.num_rows, 13)
    keep = mask_keep(mask_name, mask)
    on = np.ones(csc.num_rows, bool) if keep is None else keep
    mod = _spmspv_module(csc, mask)
    for rep, v in enumerate((v1, v2, v1)):
        got = _spmspv_run(mod, csc, v, mask_name, mask, "tiny cancelling run %d %s" % (rep, mask_name))
        assert mod.tiny_ is not None and mod.tiny_[0] == 256 and mod.tiny_[1] == 1024      # 256 entries, 1024 products: one launch
        if v is v1:
            assert np.all(got[ra] == 0) and np.array_equal(got[rb][on[rb]], q[on[rb]])
        else:
            assert np.all(got[ra][on[ra]] != 0)
        assert on[ra].any() and on[rb].any()


@pytest.mark.parametrize("kind", ["signed", "wide"])
@pytest.mark.parametrize("layout", ["general", "pattern"])
def test_signed_fold_and_row_wise(gpu, monkeypatch, layout, kind):
    """Signed and 1e-30 .. 1e30 products through the bin / fold kernels (light frontier; the one-launch path is switched off, it
    has its own test) and through the row-wise leg on the attached general / pattern plan (heavy frontier), every mask, twice
    per module."""
    set_knob(monkeypatch, "spmspv_tiny", "0")
    csr, csc, x = rmat_signed(kind, layout)
    mask = rand01(csc.num_rows, 6)
    mod = _spmspv_module(csc, mask, pull=True)
    info = mod.own_pull_.plan_.info()
    assert info["layout"] == layout and info["finite_values"]
    rng = np.random.default_rng(8)
    for density, expect in ((0.0005, "scatter"), (0.25, "row-wise")):
        v = frontier_of(x, np.flatnonzero(rng.random(csc.num_cols) < density))
        for mk in MASKS:
            for rep in range(2):
                _spmspv_run(mod, csc, v, mk, mask, "%s %s %s %s run %d" % (layout, kind, expect, mk, rep))
                assert mod.plan_.last_direction() == expect


def test_non_finite_weights_do_not_leak_through_the_row_wise_leg(gpu, monkeypatch):
    """+inf, -inf and NaN weights in columns that are NOT in the frontier: the scatter never reads them, a row-wise run would
    multiply them by the 0 it puts off the frontier (inf * 0 = NaN).  A plan records whether all its values are finite -- both
    formatters agree, info() says so -- and the operator takes the row-wise leg only then: this matrix always scatters and
    gives the oracle's result.  A light frontier that does hold an inf column gives +-inf / NaN in that column's rows."""
    set_knob(monkeypatch, "spmspv_tiny", "0")
    csr, csc, x = rmat_signed("signed", "general")
    for f in FORMATTERS:
        assert capi.SpMVPlan(csr.num_rows, csr.num_cols, csr.adj_indptr, csr.adj_indices, csr.adj_data, flags=f).info()["finite_values"]
    rng = np.random.default_rng(10)
    coldeg = np.diff(csc.adj_indptr.astype(np.int64))
    odd = np.sort(rng.choice(np.flatnonzero(coldeg >= 4), size=8, replace=False))
    ip = csc.adj_indptr.astype(np.int64)
    for k, c in enumerate(odd):
        csc.adj_data[ip[c]:ip[c + 1]] = (np.inf, -np.inf, np.nan)[k % 3]
    at = io.CSRMatrix(csc.num_cols, csc.num_rows, csc.adj_data, csc.adj_indices, csc.adj_indptr)
    back = io.csr2csc(at)                                         # the same matrix by rows
    for f in FORMATTERS:
        plan = capi.SpMVPlan(csc.num_rows, csc.num_cols, back.adj_indptr, back.adj_indices, back.adj_data, flags=f)
        assert plan.info()["layout"] == "general" and not plan.info()["finite_values"]
    mask = rand01(csc.num_rows, 6)
    mod = _spmspv_module(csc, mask, pull=True)
    assert not mod.own_pull_.plan_.info()["finite_values"]
    heavy = np.setdiff1d(np.flatnonzero(rng.random(csc.num_cols) < 0.3), odd)
    assert coldeg[heavy].sum() > csc.nnz // 8                      # (a finite matrix would go row-wise here)
    v = frontier_of(x, heavy)
    for mk in MASKS:
        for rep in range(2):
            got = _spmspv_run(mod, csc, v, mk, mask, "non-finite weights off the frontier %s run %d" % (mk, rep))
            assert np.all(np.isfinite(got)) and mod.plan_.last_direction() == "scatter"
    light = np.union1d(np.flatnonzero(rng.random(csc.num_cols) < 0.0005), odd[:2])      # an inf and a -inf column
    v = frontier_of(x, light)
    exact, _, _ = arith_expected_frontier(csc, v)
    assert np.isinf(exact).any() and 0 < (~np.isfinite(exact)).sum() < csc.num_rows // 2
    for mk in MASKS:
        _spmspv_run(mod, csc, v, mk, mask, "non-finite weights in the frontier %s" % mk)
        assert mod.plan_.last_direction() == "scatter"
