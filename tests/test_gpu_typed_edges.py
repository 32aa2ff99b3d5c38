"""GPU parity of the integer instantiations -- `unsigned` and ap_ufixed<32,8,AP_RND,AP_SAT>, six of the nine op codes of every
templated SpMV / SpMSpV kernel -- on every path the float instantiations are driven through: the structures of the general and
pattern layouts (helpers.edge_matrix / wide_matrix: hot table, row-packed records, hub rows, diagonal exceptions, bridging dummies),
split plans, both formatters, the helper / packed-vector / mix variants, row shards with and without stored entries, and the SpMSpV
paths (long columns shared by chunks, overflowing bins, the dense accumulator, tickets, odd tile heights, both cuts, the
rendezvous, row shards, one plan under changing types and zeros).  Every case asserts the structure it relies on and is BIT-EXACT
against the integer oracle (helpers.spmv_words_reference, O.spmspv_words): modular sums, or a clamped sum of non-negative rounded
products, are the same word in any order.  y is pre-filled with 0xdeadbeef.  The inputs, their shares of saturated rows and the
oracle itself are proven on the CPU in tests/test_typed_edges_cpu.py."""
import functools

import numpy as np
import pytest

from graphlily_amd import capi
from oracle import oracle as O

from helpers import (EDGE_HOT, EDGE_HUBS, EDGE_KINDS, MASKS, VALUE_TYPES, VAL_UFIXED, WORD_MAX, WORD_OPS, contended_case,
                     edge_matrix, frontier_case, long_columns_case, long_columns_csc, random_csc, rmat_csc,
                     rmat_sssp_csc, set_knob, set_plan_knobs, signed_inputs, spmv_plans, spmv_words_reference, stable_seed,
                     typed_inputs, wide_matrix, word_nonzero_zero, word_one, word_vec, word_zero)

pytestmark = pytest.mark.gpu

assert VALUE_TYPES == {"unsigned": capi.GL_VAL_UNSIGNED, "ufixed": capi.GL_VAL_UFIXED_32_8}
POISON = 0xdeadbeef


@functools.lru_cache(maxsize=None)
def _structure(which, layout):
    return edge_matrix(layout) if which == "edge" else wide_matrix()


def _words_matrix(which, layout, a):
    """The structure with the value words `a` travelling as bit patterns in the float array."""
    m = _structure(which, layout).copy()
    m.adj_data = a.view(np.float32)
    return m


def _kinds(op):
    return ("small", "large") if op == 0 else (None,)


def _inputs(which, layout, vt_name, op, kind):
    rng = np.random.default_rng(stable_seed(which, layout, vt_name, op, kind))     # (the seeds of tests/test_typed_edges_cpu.py)
    return typed_inputs(rng, _structure(which, layout), layout, VALUE_TYPES[vt_name], op, kind)


class _Run:
    """The device side of one case: x, the mask and a y that is poisoned before every run."""

    def __init__(self, rows, x, mask):
        self.rows = rows
        self.dx, self.dm, self.dy = capi.DeviceBuffer.from_host(x), capi.DeviceBuffer.from_host(mask), capi.DeviceBuffer(4 * rows)
        self.poison = np.full(rows, POISON, np.uint32)

    def __call__(self, plan, op, zero, mt, vt):
        self.dy.write(self.poison)
        plan.run_typed(self.dx, self.dm if mt else None, self.dy, op, zero, mt, vt)
        return self.dy.read(np.uint32, self.rows)


def _same(got, ref, what):
    if not np.array_equal(got, ref):
        i = np.flatnonzero(got != ref)
        raise AssertionError("%s: %d rows differ, first %s: got %s want %s" % (what, i.size, i[:8].tolist(), [hex(w) for w in got[i[:8]]],
                                                                               [hex(w) for w in ref[i[:8]]]))


# ------------------------------------------------------------------ SpMV: every structure
@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
@pytest.mark.parametrize("shape", ["unsplit", "split"])
@pytest.mark.parametrize("layout", EDGE_KINDS)
def test_every_structure(gpu, monkeypatch, layout, shape, vt_name):
    """edge_matrix in words on both formatters' plans, unsplit and split into 5 row blocks x 3 column segments: three semirings x three
    masks x both (+,x) kinds, and a non-zero `zero` without a mask.  (+,x) `large` in the fixed point is the case a split plan can
    get wrong: every unit clamps its 64-bit tile to 32 bits and the planes are added with a saturating add -- hub row 1000 sums to
    1.5 x 2^32 while each of its column segments stays below 2^32."""
    vt = VALUE_TYPES[vt_name]
    for op in WORD_OPS.values():
        for kind in _kinds(op):
            a, x, mask, zero = _inputs("edge", layout, vt_name, op, kind)
            m = _words_matrix("edge", layout, a)
            plans, split = spmv_plans(monkeypatch, "edge", layout, shape, m)       # layout, segments, hot table, hub rows, equal exports
            assert split == (shape == "split")
            run = _Run(m.num_rows, x, mask)
            ref = {mk: spmv_words_reference(m, a, x, op, vt, zero, mask, mt) for mk, mt in MASKS.items()}
            nz = word_nonzero_zero(vt, op, ref["NoMask"])
            ref_nz = spmv_words_reference(m, a, x, op, vt, nz)
            if op == 0 and kind == "large" and vt == VAL_UFIXED:
                sat = ref["NoMask"] == WORD_MAX
                assert sat.sum() >= m.num_rows // 4 and (~sat & (ref["NoMask"] != 0)).sum() >= m.num_rows // 4
                if layout == "general":
                    assert sat[EDGE_HUBS[1]] and not sat[EDGE_HUBS[0]]
            for p, fmt in zip(plans, ("host", "device")):
                what = "%s %s %s op %d %s %s" % (layout, shape, vt_name, op, kind, fmt)
                for mk, mt in MASKS.items():
                    _same(run(p, op, zero, mt, vt), ref[mk], what + " " + mk)
                _same(run(p, op, nz, 0, vt), ref_nz, what + " zero %#x" % nz)


# ------------------------------------------------------------------ SpMV: the bridging dummies of a wide cold stream
@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
@pytest.mark.parametrize("shape", ["unsplit", "split"])
@pytest.mark.parametrize("layout", ["general", "pattern"])
def test_wide_stream(gpu, monkeypatch, layout, shape, vt_name):
    """1024 x 262144 in 16 row blocks, 1 and 3 column segments: most slots of the cold stream are dummies that bridge gaps of more
    than 255 columns.  A dummy must be the identity of the value type's (+) -- 0xffffffff under (min,+), where a float +inf, a 0 or
    a wrapped sum would all be smaller than real results."""
    vt = VALUE_TYPES[vt_name]
    for op in WORD_OPS.values():
        kind = "large" if op == 0 else None
        a, x, mask, zero = _inputs("wide", layout, vt_name, op, kind)
        m = _words_matrix("wide", layout, a)
        plans, split = spmv_plans(monkeypatch, "wide", layout, shape, m)           # groups * 64 > 1.3 nnz: the dummies are there
        assert split == (shape == "split")
        run = _Run(m.num_rows, x, mask)
        for mk in ("NoMask", "WriteToZero"):
            ref = spmv_words_reference(m, a, x, op, vt, zero, mask, MASKS[mk])
            for p, fmt in zip(plans, ("host", "device")):
                _same(run(p, op, zero, MASKS[mk], vt), ref, "wide %s %s %s op %d %s %s" % (layout, shape, vt_name, op, fmt, mk))


# ------------------------------------------------------------------ SpMV: helper, packed-vector and mix variants
# (knobs, helper the general plan must report, helper the pattern plan must report, packed vector?, mix, hot table)
VARIANTS = [({"spmv_compact": 0}, "self-hot", "gather", False, None, EDGE_HOT),
            ({"spmv_compact": 1}, "self-hot", "gather", False, None, EDGE_HOT),      # (self-hot plans keep x as it is)
            ({"spmv_compact": 3}, None, None, True, None, EDGE_HOT),                 # packed even where self-hot would do
            ({"spmv_helper": 0}, "gather", "gather", True, None, EDGE_HOT),
            ({"spmv_helper": 0, "spmv_compact": 0}, "gather", "gather", False, None, EDGE_HOT),
            ({"spmv_helper": 1}, "spread", "spread", True, None, EDGE_HOT),          # spmv_spread_x_kernel<OPX, pattern>
            ({"spmv_helper": 2}, "self-hot", "gather", False, None, EDGE_HOT),
            ({"spmv_mix": 3}, None, None, None, 3, EDGE_HOT),                        # one cold + one hot element per step
            ({"spmv_mix": 0}, None, None, None, 0, 0)]                               # no hot table: cold elements only


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
@pytest.mark.parametrize("layout", ["general", "pattern"])
def test_helper_variants(gpu, monkeypatch, layout, vt_name):
    """How x reaches the kernel -- gathered by the helper (spmv_hot_gather_kernel / spmv_prescale_kernel<OPX>, which forms colval (x) x
    in the value type), spread in one pass (spmv_spread_x_kernel<OPX, pattern>), by the workgroups themselves --, with and without
    the packed vector, and the stream mixes 0 / 3: the same words whatever the variant.  info() says which one a plan took."""
    vt = VALUE_TYPES[vt_name]
    cases = []
    for op in WORD_OPS.values():
        a, x, mask, zero = _inputs("edge", layout, vt_name, op, "large" if op == 0 else None)
        m = _words_matrix("edge", layout, a)
        cases.append((op, zero, m, _Run(m.num_rows, x, mask), spmv_words_reference(m, a, x, op, vt, zero)))
    for knobs, helper_general, helper_pattern, packed, mix, hot in VARIANTS:
        for k, v in knobs.items():
            set_knob(monkeypatch, k, v)
        for op, zero, m, run, ref in cases:
            (p,), _ = spmv_plans(monkeypatch, "edge", layout, "unsplit", m, flags=(0,), hot=hot)
            info = p.info()
            helper = helper_general if layout == "general" else helper_pattern
            assert helper is None or info["helper"] == helper, (knobs, info)
            assert packed is None or (info["packed_columns"] > 0) == packed, (knobs, info)
            assert mix is None or info["mix"] == mix, (knobs, info)
            _same(run(p, op, zero, 0, vt), ref, "%s %s op %d %s" % (layout, vt_name, op, knobs))
        for k in knobs:
            set_knob(monkeypatch, k, None)


# ------------------------------------------------------------------ SpMV: row shards, one of them without stored entries
@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
@pytest.mark.parametrize("layout", ["general", "pattern"])
def test_row_shards(gpu, monkeypatch, layout, vt_name):
    """Plans of the rows [0, 97), [98, 4096) and of row 97 alone, which is empty (spmv_init_kernel<OPX>: y = mask(zero), with (||,&&)
    turning a non-zero zero into ONE): the shard's rows equal the whole matrix' result, every other word of y keeps its 0xdeadbeef."""
    vt = VALUE_TYPES[vt_name]
    set_plan_knobs(monkeypatch, "edge", "unsplit")
    for op in WORD_OPS.values():
        a, x, mask, zero = _inputs("edge", layout, vt_name, op, "large" if op == 0 else None)
        m = _words_matrix("edge", layout, a)
        n = m.num_rows
        run = _Run(n, x, mask)
        nz = word_nonzero_zero(vt, op, spmv_words_reference(m, a, x, op, vt, zero))
        refs = {(z, mk): spmv_words_reference(m, a, x, op, vt, z, mask, mt) for z in (zero, nz) for mk, mt in MASKS.items()}
        for r0, r1 in ((0, 97), (98, n), (97, 98)):
            p = capi.SpMVPlan(n, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, r0, r1)
            info = p.info()
            assert info["nnz"] == int(m.adj_indptr[r1]) - int(m.adj_indptr[r0])
            if r1 - r0 == 1:
                assert info["nnz"] == 0 and info["num_units"] == 0
            else:
                assert info["layout"] == ("general" if layout == "general" else "pattern") and p.export("hub_rows").size > 0
            for (z, mk), ref in refs.items():
                got = run(p, op, z, MASKS[mk], vt)
                what = "%s %s op %d rows [%d, %d) zero %#x %s" % (layout, vt_name, op, r0, r1, z, mk)
                _same(got[r0:r1], ref[r0:r1], what)
                assert np.all(got[:r0] == POISON) and np.all(got[r1:] == POISON), what + ": wrote outside its rows"
                if r1 - r0 == 1:      # mask(zero), spelled out
                    on = mk == "NoMask" or (mask[r0] == 0) == (mk == "WriteToZero")
                    want = 0 if not on else (word_one(vt) if z else 0) if op == 1 else z
                    assert got[r0] == want, (what, hex(got[r0]), hex(want))


# ------------------------------------------------------------------ SpMV: the typed entry point itself
def test_run_typed_entry_point(gpu, monkeypatch):
    """gl_spmv_run_typed with GL_VAL_FLOAT is gl_spmv_run, bit for bit; the bit layout and the reference-order layout serve float
    only -- an integer type is refused with GL_ERR_UNSUPPORTED before anything is written --; a GL_PLAN_NO_MULADD plan (hot table
    sized for 4-byte accumulators) serves the integer (||,&&) and (min,+)."""
    s = _structure("edge", "general")
    m = s.copy()
    m.adj_data, x = signed_inputs(np.random.default_rng(5), s, "signed")
    n = m.num_rows
    mask = (np.random.default_rng(6).integers(0, 2, size=n)).astype(np.float32)
    set_plan_knobs(monkeypatch, "edge", "unsplit")
    plan = capi.SpMVPlan(n, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data)
    dx, dm, dy = capi.DeviceBuffer.from_host(x), capi.DeviceBuffer.from_host(mask), capi.DeviceBuffer(4 * n)
    for op, zero in ((0, 0.0), (0, 0.5), (2, 255.0)):
        for mt in MASKS.values():
            plan.run(dx, dm if mt else None, dy, op, zero, mt)
            want = dy.read(np.uint32, n)
            dy.write(np.full(n, POISON, np.uint32))
            plan.run_typed(dx, dm if mt else None, dy, op, int(np.float32(zero).view(np.uint32)), mt, capi.GL_VAL_FLOAT)
            assert np.array_equal(dy.read(np.uint32, n), want) and len(np.unique(want)) > n // 4
    for vt_name, vt in VALUE_TYPES.items():
        a, xw, maskw, zero = _inputs("edge", "general", vt_name, 1, None)
        mw = _words_matrix("edge", "general", a)
        run = _Run(n, xw, maskw)
        for flag in (capi.GL_PLAN_BOOLEAN, capi.GL_PLAN_REFERENCE_ORDER):
            p = capi.SpMVPlan(n, mw.num_cols, mw.adj_indptr, mw.adj_indices, mw.adj_data, flags=flag)
            assert p.info()["layout"] == ("boolean" if flag == capi.GL_PLAN_BOOLEAN else "reference-order")
            for op in WORD_OPS.values():
                run.dy.write(run.poison)
                with pytest.raises(capi.GraphLilyError) as err:
                    p.run_typed(run.dx, None, run.dy, op, word_zero(vt, op), 0, vt)
                assert err.value.code == capi.GL_ERR_UNSUPPORTED
                assert np.all(run.dy.read(np.uint32, n) == POISON)
        for op in (1, 2):
            a, xw, maskw, zero = _inputs("edge", "general", vt_name, op, None)
            mw = _words_matrix("edge", "general", a)
            p = capi.SpMVPlan(n, mw.num_cols, mw.adj_indptr, mw.adj_indices, mw.adj_data, flags=capi.GL_PLAN_NO_MULADD)
            assert p.info()["layout"] == "general" and p.info()["hot_columns"] == EDGE_HOT
            run = _Run(n, xw, maskw)
            for mk, mt in MASKS.items():
                _same(run(p, op, zero, mt, vt), spmv_words_reference(mw, a, xw, op, vt, zero, maskw, mt), "NO_MULADD %s op %d %s" % (vt_name, op, mk))


# ------------------------------------------------------------------ SpMSpV
class _Scatter:
    """One SpMSpV plan over value words and its device buffers."""

    def __init__(self, csc, data, shard=None):
        r0, r1 = shard if shard else (0, csc.num_rows)
        self.csc, self.data, self.r0, self.r1 = csc, data, r0, r1
        self.plan = capi.SpMSpVPlan(csc.num_rows, csc.num_cols, csc.adj_indptr, csc.adj_indices, data.view(np.float32), r0, r1)
        self.dr = capi.DeviceBuffer(8 * (csc.num_rows + 1))
        self.masks = {}

    def run(self, v, mask, op, zero, mt, vt, reps=2, dtype=capi.IDX_WORD):
        """`reps` runs of one vector: the list's form is checked every time -- head {count, zero}, indices ascending and inside the
        plan's rows, no entry equal to zero -- and the densified result returned (the runs must agree)."""
        dv = capi.DeviceBuffer(8 * len(v))
        dv.write(v)
        dm = None
        if mt:
            dm = self.masks.get(id(mask))
            if dm is None:
                dm = self.masks[id(mask)] = capi.DeviceBuffer.from_host(mask)
        n, out = self.csc.num_rows, None
        for rep in range(reps):
            self.plan.run_typed(dv, dm, self.dr, op, zero, mt, vt)
            res = self.dr.read(capi.IDX_WORD, n + 1)
            cnt = int(res["index"][0])
            assert cnt <= self.r1 - self.r0 and res["val"][0] == zero, (cnt, hex(res["val"][0]))
            idx, val = res["index"][1:cnt + 1].astype(np.int64), res["val"][1:cnt + 1]
            assert np.all(np.diff(idx) > 0), "result indices must be ascending and unique"
            assert cnt == 0 or (idx[0] >= self.r0 and idx[-1] < self.r1)
            assert not np.any(val == zero), "entries equal to zero must not be emitted"
            dense = np.full(n, zero, np.uint32)
            dense[idx] = val
            assert out is None or np.array_equal(out, dense), "run %d differs from the run before it" % rep
            out = dense
        return out

    def check(self, v, mask, op, zero, mk, vt, what):
        mt = MASKS[mk]
        got = self.run(v, mask, op, zero, mt, vt)
        ref = O.spmspv_words(self.csc.adj_indptr, self.csc.adj_indices, self.data, v, self.csc.num_rows, op, vt, zero, mask if mt else None, mt)
        if self.r0 or self.r1 != self.csc.num_rows:
            ref[:self.r0] = zero
            ref[self.r1:] = zero
        _same(got, ref, "%s %s" % (what, mk))
        return got


@pytest.mark.parametrize("sem", list(WORD_OPS))
@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_long_columns_then_overflow(gpu, vt_name, sem):
    """24 columns of 4097 .. 8191 entries, all in the frontier: shared between workgroups by chunks (bin_chunk).  Then every column
    named twice: the bins, sized for one visit, overflow into the dense accumulator (spill_one: a clamped compare-and-swap loop for
    the fixed point's (+,x), a wrapping atomic add for unsigned, the integer atomic min) and the fold merges bin and accumulator --
    rows that saturate only with both parts together are there.  Then the first vector again: nothing is left behind."""
    vt, op = VALUE_TYPES[vt_name], WORD_OPS[sem]
    csc, data, vs, mask, zero = long_columns_case(vt_name, op)
    s = _Scatter(csc, data)
    res = [[s.check(v, mask, op, zero, mk, vt, "long columns %s %s vector %d" % (vt_name, sem, k)) for mk in ("NoMask", "WriteToOne")]
           for k, v in enumerate(vs)]
    assert np.array_equal(res[0][0], res[2][0])
    if op == 0 and vt == VAL_UFIXED:
        assert ((res[0][0] != WORD_MAX) & (res[1][0] == WORD_MAX)).sum() >= csc.num_rows // 20


@pytest.mark.parametrize("sem", list(WORD_OPS))
@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_everything_through_the_dense_accumulator(gpu, monkeypatch, vt_name, sem):
    """131136 rows in tiles of 64 are 2049 tiles, one more than the bin kernel has counters for: every product is a global atomic on
    the dense accumulator and the fold reads all of it.  Rows 0 and 1 occur in every 4th column -- hundreds of contended
    compare-and-swap adds; in the fixed point row 0 saturates and row 1 does not."""
    vt, op = VALUE_TYPES[vt_name], WORD_OPS[sem]
    set_knob(monkeypatch, "spmspv_tile_rows", 64)
    csc, data, vs, mask, zero = contended_case(vt_name, op)
    assert csc.num_rows == 2049 * 64
    s = _Scatter(csc, data)
    for v in vs:
        got = {mk: s.check(v, mask, op, zero, mk, vt, "dense accumulator %s %s %d" % (vt_name, sem, int(v["index"][0])))
               for mk in ("NoMask", "WriteToZero")}
        if op == 0 and vt == VAL_UFIXED:
            assert got["NoMask"][0] == WORD_MAX and 0 < got["NoMask"][1] < WORD_MAX


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
@pytest.mark.parametrize("tile_rows", [64, 192])
def test_many_tiles_binned(gpu, monkeypatch, tile_rows, vt_name):
    """40000 rows in tiles of 64 (625 tiles: handed out by ticket) and of 192 (not a power of two: row -> tile by multiplication),
    three hub columns of 5000 entries; vectors of 300 and 3000 entries (every workgroup cuts the products itself, direct and
    sorted batches) and of a third of the columns (the rendezvous)."""
    vt = VALUE_TYPES[vt_name]
    set_knob(monkeypatch, "spmspv_tile_rows", tile_rows)
    csc = random_csc(40000, 6, 5, (3, 5000))
    for sem, op in WORD_OPS.items():
        data, vs, mask, zero = frontier_case(csc, "tiles", vt_name, op, (300, 3000, 40000 // 3))
        s = _Scatter(csc, data)
        for v in vs:
            for mk in ("NoMask", "WriteToZero"):
                s.check(v, mask, op, zero, mk, vt, "tiles of %d %s %s %d" % (tile_rows, vt_name, sem, int(v["index"][0])))


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_both_cuts(gpu, monkeypatch, vt_name):
    """Mid-size vectors over a matrix without long columns, cut into equal slices of entries and -- forced by the knob -- into equal
    ranges of products behind the rendezvous: the same list both ways, the oracle's."""
    vt = VALUE_TYPES[vt_name]
    csc = rmat_sssp_csc()
    for sem, op in WORD_OPS.items():
        data, vs, mask, zero = frontier_case(csc, "cuts", vt_name, op, (4097, 9000))
        s = _Scatter(csc, data)
        for v in vs:
            for mk in ("NoMask", "WriteToOne"):
                lists = []
                for maxcol in (1 << 30, 0):                               # by entries; by products
                    set_knob(monkeypatch, "spmspv_by_entries_maxcol", maxcol)
                    lists.append(s.check(v, mask, op, zero, mk, vt, "cut %d %s %s %d" % (maxcol, vt_name, sem, int(v["index"][0]))))
                set_knob(monkeypatch, "spmspv_by_entries_maxcol", None)
                assert np.array_equal(lists[0], lists[1])


def test_one_plan_changing_type_and_zero(gpu):
    """The dense accumulator is all `zero` between runs and is refilled when the zero's BITS change: float 255.0, the fixed point's
    255 << 24 and unsigned 0xffffffff are three words for "the (min,+) zero", 0.0 and the integer 0 are one.  One plan whose
    values are 1.0, 2.0 and 3.0 as floats (63.5, 64.0 and 64.25 in the fixed point) runs the doubled long-column frontier --
    every run spills -- under seven type / semiring / zero combinations in a row, each against its own oracle; the float runs
    hold small integers, so they are exact as well."""
    csc, cols = long_columns_csc()
    rng = np.random.default_rng(23)
    fdata = rng.integers(1, 4, size=csc.nnz).astype(np.float32)
    data = fdata.view(np.uint32)
    s = _Scatter(csc, data)
    both = np.concatenate([cols, cols])
    U, F = VALUE_TYPES["unsigned"], VAL_UFIXED
    oc = O.CSC(csc.num_rows, csc.num_cols, fdata, csc.adj_indices, csc.adj_indptr)
    steps = [("float", 0, 0.0), (F, 2, 255 << 24), (U, 2, WORD_MAX), (F, 0, 0), (U, 1, 0), ("float", 2, 255.0), (F, 0, 0)]
    spilled_and_clamped = 0
    for k, (vt, op, zero) in enumerate(steps):
        if vt == "float":
            xv = rng.integers(1, 5, size=len(both)).astype(np.float32)
            v = O.make_sparse_vec(both, xv)
            zbits = int(np.float32(zero).view(np.uint32))
            got = s.run(v.view(capi.IDX_WORD), None, op, zbits, 0, capi.GL_VAL_FLOAT)
            ref = O.spmspv(oc, v, op, zero)
            _same(got, ref.view(np.uint32), "step %d float op %d" % (k, op))
            assert (ref != np.float32(zero)).sum() > csc.num_rows // 4
        else:
            hi = {0: 1 << 23, 1: 1 << 20, 2: 120 << 24}[op]
            xv = rng.integers(0, hi, size=len(both), dtype=np.uint64).astype(np.uint32)
            xv[::7] = 0xfffffff0 if op == 2 else 0
            v = word_vec(both, xv)
            got = s.check(v, None, op, zero, "NoMask", vt, "step %d type %d op %d" % (k, vt, op))
            assert (got != zero).sum() > csc.num_rows // 4
            if op == 0:
                spilled_and_clamped += int((got == WORD_MAX).sum() > 0 and ((got != WORD_MAX) & (got != 0)).sum() > 0)
    assert spilled_and_clamped == 2


@pytest.mark.parametrize("vt_name", list(VALUE_TYPES))
def test_row_shards_concatenate(gpu, vt_name):
    """Row-sharded plans produce disjoint ascending slices of the full result; and an empty frontier gives count 0 behind a head
    that holds the zero word, on a plan that has just run."""
    vt = VALUE_TYPES[vt_name]
    csc = rmat_csc()
    n, cut = csc.num_rows, 9984
    for sem, op in WORD_OPS.items():
        data, (v,), mask, zero = frontier_case(csc, "shards", vt_name, op, (1000,))
        full = _Scatter(csc, data).check(v, mask, op, zero, "WriteToZero", vt, "whole %s %s" % (vt_name, sem))
        lo = _Scatter(csc, data, (0, cut))
        a = lo.check(v, mask, op, zero, "WriteToZero", vt, "rows [0, %d) %s %s" % (cut, vt_name, sem))
        b = _Scatter(csc, data, (cut, n)).check(v, mask, op, zero, "WriteToZero", vt, "rows [%d, %d) %s %s" % (cut, n, vt_name, sem))
        assert np.all(a[cut:] == zero) and np.all(b[:cut] == zero) and (a[:cut] != zero).any() and (b[cut:] != zero).any()
        assert np.array_equal(np.concatenate([a[:cut], b[cut:]]), full)
        for mk in MASKS:
            got = lo.run(word_vec([], []), mask, op, zero, MASKS[mk], vt)          # (run() checks count <= rows, head value == zero)
            assert np.all(got == zero)
            res = lo.dr.read(capi.IDX_WORD, 1)
            assert int(res["index"][0]) == 0 and res["val"][0] == zero
