"""Shared helpers for the parity tests (the oracle is the checker, never the thing under test)."""
import functools
import os
import subprocess

import numpy as np

from graphlily_amd import datasets, io
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "graphlily_amd", "lib")


def build_cpp_driver(source, *defines):
    """tests/cpp/<source> against include/, warnings as errors, linked to the HIP library -> the executable's path:
    build/<source's stem>, followed by _<DEFINE> for every -D<...>_<DEFINE> given (typed_modules_driver_UFIXED)"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "_".join([source[:-len(".cpp")]] + [d.rsplit("_", 1)[-1] for d in defines]))
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror"] + list(defines) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", source), "-o", exe,
                           "-L", LIBDIR, "-lgraphlily_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def to_oracle(m):
    cls = O.CSC if isinstance(m, io.CSCMatrix) else O.CSR
    return cls(m.num_rows, m.num_cols, m.adj_data, m.adj_indices, m.adj_indptr)


def rand01(n, seed):
    """The reference draws x and masks as rand() % 2 (tests/test_module_spmv_spmspv.cpp:105-111);
    seeded here."""
    return np.random.default_rng(seed).integers(0, 2, size=n).astype(np.float32)


def named_matrix(name):
    if name == "dense_32":
        return datasets.dense(32)
    if name == "dense_1K":
        return datasets.dense(1024)
    if name == "uniform_10K_10":
        return datasets.uniform(10000, 10, seed=7)
    if name == "rmat_20K":          # power-law: a few rows far longer than a tile, many empty rows
        return datasets.rmat(20000, 400000, seed=11, symmetric=False)
    if name == "rmat_sym_50K":
        return datasets.rmat(50000, 1500000, seed=12, symmetric=True)
    if name == "gplus_small":       # googleplus stand-in at 1/8 scale
        return datasets.paper_graph("googleplus", scale=0.125)
    raise KeyError(name)


def spmv_prepare(name, row_div=128, col_div=8):
    """Matrix preparation of the reference SpMV test (tests/test_module_spmv_spmspv.cpp:144-151):
    pad rows to num_hbm_channels*pack_size and cols to pack_size, values = 1/num_rows."""
    m = named_matrix(name)
    io.util_round_csr_matrix_dim(m, row_div, col_div)
    m.adj_data = np.full(m.adj_data.shape[0], np.float32(1.0 / m.num_rows), dtype=np.float32)
    return m


SEMIRINGS = {"Arithmetic": (0, 0.0), "Logical": (1, 0.0), "Tropical": (2, 255.0), "TropicalFloatInf": (2, 999999999.0)}
MASKS = {"NoMask": 0, "WriteToZero": 1, "WriteToOne": 2}


U32 = 2.0 ** -24   # fp32 unit roundoff


def arith_exact(m, x, rows=None):
    """float64 evaluation of the (+,x) product and the per-row data the float tolerance needs:
    exact[r] = sum a_i x_i, abs_sum[r] = sum |a_i x_i|, length[r]."""
    n = m.nnz
    prod = m.adj_data[:n].astype(np.float64) * np.asarray(x, np.float64)[m.adj_indices[:n]]
    lens = np.diff(m.adj_indptr.astype(np.int64))
    row_of = np.repeat(np.arange(m.num_rows), lens)
    exact = np.bincount(row_of, weights=prod, minlength=m.num_rows)
    abs_sum = np.bincount(row_of, weights=np.abs(prod), minlength=m.num_rows)
    return exact, abs_sum, lens


def assert_arith_parity(got, ref, exact, abs_sum, lens, what="", keep=None):
    """Float (+,x) tolerance, stated in full:
      (1) |got - exact| <= 1e-5 |exact| (+ 4u abs_sum for cancellation): the HIP result is within the
          north_star's 1e-5 relative of the exactly evaluated product;
      (2) |got - ref| <= 1e-5 |ref| + L u abs_sum: against the fp32 oracle, whose sequential
          accumulation (spmv_module.h:495) itself carries the classical forward error (L-1) u sum|a_i x_i|
          -- on rows with thousands of entries that alone exceeds 1e-5, whatever order the device uses.
    `keep` selects the rows that were not masked off (masked rows must be exactly 0)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if keep is None:
        keep = np.ones(got.shape[0], bool)
    if np.any(got[~keep] != 0):
        raise AssertionError("%s: masked-off rows must be exactly 0" % what)
    e1 = np.abs(got - exact) - (1e-5 * np.abs(exact) + 4 * U32 * abs_sum)
    e2 = np.abs(got - ref) - (1e-5 * np.abs(ref) + np.maximum(lens, 1) * U32 * abs_sum)
    for name, e in (("vs exact", e1), ("vs oracle", e2)):
        bad = np.nonzero((e > 0) & keep)[0]
        if bad.size:
            i = bad[0]
            raise AssertionError("%s %s: %d rows out of tolerance, first row %d (len %d): got %r ref %r exact %r" %
                                 (what, name, bad.size, i, lens[i], got[i], ref[i], exact[i]))


def assert_parity(got, ref, op, what=""):
    """Bit-exact for the boolean and (min,+) semirings.  For float (+,x) this short form is the
    1e-5 relative bar of the north_star and is only used where rows are short; long-row cases go
    through assert_arith_parity."""
    got = np.asarray(got, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    if op == 0:
        ok = np.allclose(got, ref, rtol=1e-5, atol=1e-9)
        if not ok:
            bad = np.nonzero(~np.isclose(got, ref, rtol=1e-5, atol=1e-9))[0]
            raise AssertionError("%s: %d mismatches, first at %d: got %r ref %r" %
                                 (what, bad.size, bad[0], got[bad[0]], ref[bad[0]]))
    else:
        if not np.array_equal(got, ref):
            bad = np.nonzero(got != ref)[0]
            raise AssertionError("%s: %d mismatches (bit-exact required), first at %d: got %r ref %r" %
                                 (what, bad.size, bad[0], got[bad[0]], ref[bad[0]]))


def set_knob(monkeypatch, key, value):
    """One planner override of GRAPHLILY_DEBUG="key=value,..." (csrc/gl_spmv_plan.h debug_knob: test hooks that force a decision
    the planner would take from the matrix -- plan shape, hot table, helper mode, tile height ...); value None removes the key."""
    import os
    cur = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    if value is None:
        cur.pop(key, None)
    else:
        cur[key] = str(value)
    if cur:
        monkeypatch.setenv("GRAPHLILY_DEBUG", ",".join("%s=%s" % kv for kv in cur.items()))
    else:
        monkeypatch.delenv("GRAPHLILY_DEBUG", raising=False)


# ------------------------------------------------------------------ matrices that reach every structure of the SpMV layouts
def csr_from_coo(n_rows, n_cols, rows, cols, data=None):
    """CSR of (row, col) pairs that are already grouped by ascending row; values default to 1."""
    indptr = np.zeros(n_rows + 1, np.uint32)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    if data is None:
        data = np.ones(len(rows), np.float32)
    return io.CSRMatrix(n_rows, n_cols, np.asarray(data, np.float32), np.asarray(cols).astype(np.uint32), indptr)


def record_boundary_coo(rng, n, hotc, cold_cols=None, empty_every=0):
    """Row r holds r % 17 of the `hotc` hot columns (0, 1, 7, 8, 14, 15 among the counts: an empty, a padded, an exactly full
    record of the row-packed hot stream, one over) and three cold ones drawn from `cold_cols` (default: every other column);
    every `empty_every`-th row stays empty."""
    if cold_cols is None:
        cold_cols = hotc + np.arange(n - hotc)
    rows, cols = [], []
    for r in range(n):
        if empty_every and r % empty_every == 0:
            continue
        k = r % 17
        hot = (np.arange(k) * 5 + r) % hotc                      # k distinct hot columns (5 is coprime to 64)
        cold = cold_cols[rng.choice(len(cold_cols), size=3, replace=False)]
        c = np.unique(np.concatenate([hot, cold]))
        rows.append(np.full(c.shape[0], r))
        cols.append(c)
    return np.concatenate(rows), np.concatenate(cols)


def hub_rows_coo(rng, n, dense_rows, others=3, from_cols=None):
    """`dense_rows` hold n / 2 entries each (hub rows: the 16 private LDS slots), every other row `others` (0: none)."""
    if from_cols is None:
        from_cols = np.arange(n)
    rows, cols = [], []
    for r in range(n):
        k = n // 2 if r in dense_rows else others
        if k == 0:
            continue
        rows.append(np.full(k, r))
        cols.append(np.sort(from_cols[rng.choice(len(from_cols), size=k, replace=False)]))
    return np.concatenate(rows), np.concatenate(cols)


EDGE_HOT = 64                    # hot columns of edge_matrix (the tests set the planner's table to this size)
EDGE_HUBS = (7, 1000, 4095)
EDGE_KINDS = ("general", "pattern", "pattern_diag")


def edge_matrix(kind, n=4096):
    """One small matrix that reaches every structure of the general / pattern layouts: 64 hot columns with r % 17 hot entries
    in row r next to 3 cold ones, the hub rows EDGE_HUBS of n / 2 entries, every 97th row empty, column n - 2 empty, column
    n - 1 in every 64th row (from row 5 on) and a diagonal entry in every third row.  `kind`: `general` per-entry values, `pattern`
    column-constant ones, `pattern_diag` column-constant ones with a differing diagonal that is negative on half of its
    rows; all signed (signed_inputs replaces them by the other value kinds on the same structure)."""
    assert kind in EDGE_KINDS
    rng = np.random.default_rng(97)
    usable = np.arange(EDGE_HOT, n - 2)                      # cold columns: neither n - 2 (stays empty) nor n - 1
    r0, c0 = record_boundary_coo(rng, n, EDGE_HOT, cold_cols=usable, empty_every=97)
    r1, c1 = hub_rows_coo(rng, n, EDGE_HUBS, others=0, from_cols=np.delete(np.arange(n), n - 2))
    last = np.arange(5, n, 64)
    last = last[last % 97 != 0]
    diag = np.arange(0, n, 3)
    diag = diag[(diag % 97 != 0) & (diag != n - 2)]
    key = np.unique(np.concatenate([r0 * n + c0, r1 * n + c1, last * n + (n - 1), diag * n + diag]).astype(np.int64))
    m = csr_from_coo(n, n, key // n, key % n)
    m.adj_data, _ = signed_inputs(np.random.default_rng(98), m, "signed", layout=kind)
    return m


def wide_matrix():
    """1024 x 262144 with 4 sorted random columns per row: with spmv_blocks=16 most gaps of the delta-coded cold stream exceed
    255 columns and are bridged by dummy entries (the smallest shape at which that holds)."""
    rng = np.random.default_rng(77)
    rows, cols, deg = 1024, 262144, 4
    indices = np.sort(rng.integers(0, cols, size=(rows, deg)), axis=1).astype(np.uint32).reshape(-1)
    return io.CSRMatrix(rows, cols, np.ones(rows * deg, np.float32), indices, np.arange(0, rows * deg + 1, deg, dtype=np.uint32))


def edge_poison(m, layout, a):
    """{column: non-finite x} for edge_matrix with the values `a`: the hot columns 3 and 8 with signs such that a row holding
    both expects inf - inf = NaN whatever the layout (column-constant values give every such row the same two signs), a cold
    column, the empty column n - 2 (a NaN there must reach no row), column n - 1, a cold column of a hub row and, for
    pattern_diag, a column whose diagonal entry is an exception."""
    n = m.num_cols
    ip, ix = m.adj_indptr.astype(np.int64), m.adj_indices
    cold_of = lambda r: int([c for c in ix[ip[r]:ip[r + 1]] if EDGE_HOT <= c < n - 2 and c != r][0])
    both = [r for r in range(EDGE_HOT, n) if r not in EDGE_HUBS and {3, 8} <= set(ix[ip[r]:ip[r + 1]].tolist())][0]
    e3, e40 = (ip[both] + list(ix[ip[both]:ip[both + 1]]).index(c) for c in (3, 8))
    p = {3: np.inf, 8: np.inf * -np.sign(a[e3]) * np.sign(a[e40]), cold_of(1): -np.inf, n - 2: np.nan, n - 1: np.inf,
         cold_of(EDGE_HUBS[1]): np.nan}
    if layout == "pattern_diag":
        p[300] = -np.inf          # row 300 holds a diagonal entry (300 % 3 == 0, 300 % 97 != 0)
    return p


def wide_poison(m, a):
    """{column: non-finite x} for wide_matrix with the values `a`: the first column of every 16th row, +inf / -inf / NaN in
    turn, the second column of row 0 with the sign that makes the row inf - inf, and a NaN in a column no row holds."""
    ix = m.adj_indices
    p = {}
    for k, r in enumerate(range(0, m.num_rows, 16)):
        p[int(ix[4 * r])] = (np.inf, -np.inf, np.nan)[k % 3]
    p[int(ix[1])] = np.inf * -np.sign(a[0]) * np.sign(a[1])
    unused = np.setdiff1d(np.arange(1000), ix[:m.nnz])
    p[int(unused[0])] = np.nan
    return p


def _signs(rng, n):
    return np.where(rng.integers(0, 2, size=n) > 0, 1.0, -1.0)


def signed_inputs(rng, m, kind, layout="general", poison=None):
    """(adj_data, x) for the CSR m.  Kinds: `signed` a, x uniform in [-1, 1); `cancelling` (general layout) x signed with
    |x| in [0.5, 2) and a_i = s_i c_r / x[col_i], s_i = +1, -1, ... along the row, c_r in [1, 2): the products are +-c_r up to
    one rounding; `wide` a, x = +-10^U(-15, 15); `subnormal` |a| in [1e-25, 1e-20], |x| in [1e-20, 1e-18] (log-uniform):
    every product is subnormal or underflows; `poison` = `signed` with x[c] = v for the {c: v} that `poison(a)` returns.
    layout `pattern`: the values are drawn per column (a = colval[col]); `pattern_diag`: so, and the diagonal entries get
    values of their own, negative on every second row that holds one."""
    nnz, nc = m.nnz, m.num_cols
    ip = m.adj_indptr.astype(np.int64)
    col = m.adj_indices[:nnz].astype(np.int64)
    row = np.repeat(np.arange(m.num_rows), np.diff(ip))
    count = nnz if layout == "general" else nc

    def draw(k, lo, hi):          # +-10^U(lo, hi)
        return _signs(rng, k) * 10.0 ** rng.uniform(lo, hi, size=k)

    if kind in ("signed", "poison"):
        a, x = rng.uniform(-1, 1, size=count), rng.uniform(-1, 1, size=nc)
        dg = lambda k: rng.uniform(0.25, 1, size=k)
    elif kind == "wide":
        a, x = draw(count, -15, 15), draw(nc, -15, 15)
        dg = lambda k: 10.0 ** rng.uniform(-15, 15, size=k)
    elif kind == "subnormal":
        a, x = draw(count, -25, -20), draw(nc, -20, -18)
        dg = lambda k: 10.0 ** rng.uniform(-25, -20, size=k)
    elif kind == "cancelling":
        assert layout == "general", "a cancelling row needs per-entry values"
        x = _signs(rng, nc) * rng.uniform(0.5, 2, size=nc)
        x = x.astype(np.float32)
        c_r = rng.uniform(1, 2, size=m.num_rows)
        sigma = np.where((np.arange(nnz) - ip[row]) % 2 == 0, 1.0, -1.0)
        a = (sigma * c_r[row]).astype(np.float32) / x[col]
    else:
        raise KeyError(kind)
    a, x = np.asarray(a, np.float32), np.asarray(x, np.float32)
    if layout != "general":
        a = a[col]
        if layout == "pattern_diag":
            d = np.flatnonzero(col == row)
            mag = dg(len(d))
            a = a.copy()
            a[d] = (mag * np.where(np.arange(len(d)) % 2 == 0, -1.0, 1.0)).astype(np.float32)
    if kind == "poison":
        for c, v in poison(a).items():
            x[c] = v
    return np.ascontiguousarray(a, np.float32), x


# ------------------------------------------------------------------ the (+,x) reference and its derived bounds
def _arith_rows(row_of, a, xv, num_rows):
    with np.errstate(all="ignore"):
        p = np.asarray(a, np.float32) * np.asarray(xv, np.float32)       # the one rounding oracle and device both do
        p64 = p.astype(np.float64)
        exact = np.bincount(row_of, weights=p64, minlength=num_rows)     # inf / NaN propagate, inf + -inf = NaN
        abs_sum = np.bincount(row_of, weights=np.where(np.isfinite(p64), np.abs(p64), 0.0), minlength=num_rows)
    lens = np.bincount(row_of, minlength=num_rows)
    return exact, abs_sum, lens


def arith_expected(m, x):
    """The (+,x) product of the CSR m: p = f32(a) * f32(x[col]) in float32 (numpy keeps subnormals), exact[r] = sum p in
    float64, abs_sum[r] = sum |p| over the finite p, lens[r] -> (exact, abs_sum, lens)."""
    n = m.nnz
    row_of = np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64)))
    return _arith_rows(row_of, m.adj_data[:n], np.asarray(x, np.float32)[m.adj_indices[:n]], m.num_rows)


def arith_expected_frontier(csc, v):
    """arith_expected of the product restricted to the columns the sparse vector v names (columns off the frontier are never
    read, whatever they hold; a column named twice is applied twice)."""
    cnt = int(v["index"][0])
    cols, xv = v["index"][1:cnt + 1].astype(np.int64), v["val"][1:cnt + 1]
    ip = csc.adj_indptr.astype(np.int64)
    lens = ip[cols + 1] - ip[cols]
    pos = np.repeat(ip[cols] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
    return _arith_rows(csc.adj_indices[pos].astype(np.int64), csc.adj_data[pos], np.repeat(xv, lens), csc.num_rows)


def _assert_arith(got, exp, bound, lens, keep, what):
    got = np.asarray(got, np.float64)
    assert got.shape == exp.shape, "%s: shape %s vs %s" % (what, got.shape, exp.shape)
    if keep is None:
        keep = np.ones(got.shape[0], bool)
    off = ~keep
    if np.any(got[off] != 0) or np.any(np.isnan(got[off])):
        raise AssertionError("%s: masked-off rows must be the literal 0" % what)
    nan, inf = np.isnan(exp) & keep, np.isinf(exp) & keep
    fin = keep & ~nan & ~inf
    with np.errstate(all="ignore"):
        bad = (nan & ~np.isnan(got)) | (inf & (got != exp)) | (fin & ~(np.abs(got - exp) <= bound))
    bad = np.flatnonzero(bad)
    if bad.size:
        i = bad[0]
        raise AssertionError("%s: %d rows wrong, first row %d (len %d): got %r expected %r bound %r" %
                             (what, bad.size, i, lens[i], got[i], exp[i], bound[i]))


def assert_arith_signed(got, exp, abs_sum, lens, split, keep=None, what=""):
    """Every row of a (+,x) SpMV result against arith_expected.  Masked-off rows are the literal 0, rows that expect NaN hold
    a NaN, rows that expect +-inf hold it, every other row is within
        u |exp| + (u if split) abs_sum + lens 2^-52 abs_sum + 2^-149,   u = 2^-24:
    the device sum is an f64 sum of the same f32 products in some order (lens 2^-52 abs_sum covers its rounding and that of
    the expectation) rounded once to f32; split plans round each segment's partial sum to f32 first (at most abs_sum large)
    and add the planes in f64.  2^-149: the rounding of a subnormal result.  Derived, not measured."""
    with np.errstate(all="ignore"):
        bound = U32 * np.abs(exp) + (U32 if split else 0.0) * abs_sum + lens * 2.0 ** -52 * abs_sum + 2.0 ** -149
    _assert_arith(got, exp, bound, lens, keep, what)


def assert_arith_scatter(got, exp, abs_sum, lens, keep=None, what=""):
    """The same with the bound of an f32 sum in any order, lens u abs_sum + u |exp| + 2^-149: the SpMSpV paths (global f32
    atomics, mixed LDS / global folds) and either side against the fp32 oracle."""
    with np.errstate(all="ignore"):
        bound = lens * U32 * abs_sum + U32 * np.abs(exp) + 2.0 ** -149
    _assert_arith(got, exp, bound, lens, keep, what)


def mask_keep(mask_name, mask, ref=0.0):
    """Rows a mask leaves on (None: all), compared with `ref` (SpMV: 0, SpMSpV: the semiring's zero)."""
    if MASKS[mask_name] == O.WRITETOZERO:
        return np.asarray(mask) == np.float32(ref)
    if MASKS[mask_name] == O.WRITETOONE:
        return np.asarray(mask) != np.float32(ref)
    return None


def stable_seed(*names):
    """A seed that depends on the case's names only (not on Python's per-process string hashing)."""
    import zlib
    return zlib.crc32("/".join(str(n) for n in names).encode())


def min_plus_inputs(rng, m, zero, layout="general"):
    """(adj_data, x) for (min,+): weights are signed eighths in [-8, 8] with -0.0 and 0.0 among them (per entry, per column, or
    per column with a differing diagonal); x is finite in [-50, 50], the semiring's zero on half of the columns, +inf on a few
    and -inf on a few.  No weight is non-finite, so no product is a NaN."""
    nnz, nc = m.nnz, m.num_cols
    col = m.adj_indices[:nnz].astype(np.int64)
    row = np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64)))
    count = nnz if layout == "general" else nc
    a = (rng.integers(-64, 65, size=count) / 8.0).astype(np.float32)
    a[rng.integers(0, count, size=max(count // 16, 2))] = np.float32(-0.0)
    a[rng.integers(0, count, size=max(count // 16, 2))] = np.float32(0.0)
    if layout != "general":
        colval, a = a, a[col]
        if layout == "pattern_diag":
            d = np.flatnonzero(col == row)
            mag = np.abs(colval[col[d]])
            a[d] = np.where(mag > 7.5, mag - np.float32(0.5), mag + np.float32(0.5)) * np.where(np.arange(len(d)) % 2 == 0, np.float32(-1), np.float32(1))
    x = rng.uniform(-50, 50, size=nc).astype(np.float32)
    x[rng.random(nc) < 0.5] = np.float32(zero)
    x[rng.integers(0, nc, size=max(nc // 100, 3))] = np.inf
    x[rng.integers(0, nc, size=max(nc // 100, 3))] = -np.inf
    return np.ascontiguousarray(a, np.float32), x


ODD_VALUES = np.array([1.0, 0.0, -0.0, -3.5, np.nan, 2.0, np.inf, -np.inf, 1e-40], np.float32)
ODD_X = np.array([0.0] * 8 + [1.0, -0.0, np.nan, -2.0, np.inf, -np.inf, 1e-40], np.float32)
ODD_MASK = np.array([0.0, 0.0, 1.0, 1.0, -0.0, np.nan, -1.0, np.inf, 1e-40], np.float32)


def logical_odd_inputs(rng, m, layout="general"):
    """(adj_data, x, mask) for (||,&&) on floats: explicit zeros, -0.0, NaN, negatives, +-inf and a subnormal in the weights
    (per entry, or per column: some columns are all NaN, bitwise equal), in x and in the mask."""
    nnz = m.nnz
    if layout == "general":
        a = rng.choice(ODD_VALUES, size=nnz)
    else:
        colval = rng.choice(ODD_VALUES, size=m.num_cols)
        a = colval[m.adj_indices[:nnz].astype(np.int64)]
    return np.ascontiguousarray(a, np.float32), rng.choice(ODD_X, size=m.num_cols), rng.choice(ODD_MASK, size=m.num_rows)


def cancelling_csc(n=4096, frontier=256):
    """An n x n CSC with 4 entries per column and two sparse vectors over the same `frontier` columns (4 * frontier products:
    the one-workgroup SpMSpV path).  The frontier columns come in groups of four, A B C D, and every group has two rows
    of its own: row ra receives w x from A and -w x from B and nothing else -- it cancels to the fill value --, row rb receives
    u x, -u x and a third product q from C -- it returns to the fill value and is reached again.  w, u, x and q are small
    dyadic rationals, so these sums are exact in any order.  All other entries are signed random floats in rows outside the
    ra / rb.  The second vector doubles x on the B columns: nothing cancels any more.
    -> (csc, v1, v2, ra, rb, q)"""
    rng = np.random.default_rng(4096)
    assert frontier % 4 == 0
    g = frontier // 4
    rows = np.stack([rng.choice(n, size=4, replace=False) for _ in range(n)])
    vals = rng.uniform(-1, 1, size=(n, 4)).astype(np.float32)
    special = rng.choice(n, size=2 * g, replace=False)
    ra, rb = special[:g], special[g:]
    plain = np.setdiff1d(np.arange(n), special)
    fcols = np.sort(rng.choice(n, size=frontier, replace=False))
    for c in fcols:                                               # frontier columns reach the special rows only on purpose
        rows[c] = plain[rng.choice(len(plain), size=4, replace=False)]
    x = np.zeros(n, np.float32)
    x[fcols] = rng.uniform(-1, 1, size=frontier)
    q = np.zeros(g, np.float32)
    for j in range(g):
        A, B, C = fcols[4 * j], fcols[4 * j + 1], fcols[4 * j + 2]
        w, u, t = (rng.integers(1, 17, size=3) * rng.choice([-1, 1], size=3) / 8.0).astype(np.float32)
        x[A] = x[B] = np.float32(rng.integers(1, 9) / 4.0)
        x[C] = np.float32(-rng.integers(1, 9) / 4.0)
        rows[A, :2], vals[A, :2] = (ra[j], rb[j]), (w, u)
        rows[B, :2], vals[B, :2] = (ra[j], rb[j]), (-w, -u)
        rows[C, 0], vals[C, 0] = rb[j], t
        q[j] = t * x[C]
    order = np.argsort(rows, axis=1)
    rows, vals = np.take_along_axis(rows, order, 1), np.take_along_axis(vals, order, 1)
    csc = io.CSCMatrix(n, n, vals.reshape(-1), rows.reshape(-1).astype(np.uint32), np.arange(0, 4 * n + 1, 4, dtype=np.uint32))
    x2 = x.copy()
    x2[fcols[1::4]] *= 2
    sv = lambda xs: O.make_sparse_vec(fcols.astype(np.uint32), xs[fcols])
    return csc, sv(x), sv(x2), ra, rb, q


def rmat_signed(kind, layout):
    """rmat_20K with signed values of `kind` (signed / wide), per entry (`general`) or per column (`pattern`)
    -> (csr, csc, x): x is dense, a frontier takes its entries."""
    m = named_matrix("rmat_20K")
    m.adj_data, x = signed_inputs(np.random.default_rng(stable_seed("rmat", kind, layout)), m, kind, layout=layout)
    return m, io.csr2csc(m), x


def frontier_of(x, idx):
    idx = np.asarray(idx, np.uint32)
    return O.make_sparse_vec(idx, np.asarray(x, np.float32)[idx])


def checked_sparse_result(mod, zero, num_rows):
    """A SpMSpV module's result list, checked for this build's documented form -- ascending unique indices, head {nnz, zero},
    no emitted value equal to zero -- and densified."""
    from graphlily_amd import module as M
    res = mod.send_results_device_to_host()
    nnz = mod.get_results_nnz()
    assert nnz == int(res["index"][0])
    idx = res["index"][1:nnz + 1].astype(np.int64)
    assert np.all(np.diff(idx) > 0), "result indices must be ascending and unique"
    assert res["val"][0] == np.float32(zero)          # head {nnz, Zero} (kernel_spmspv_impl.h:551-555)
    assert not np.any(res["val"][1:nnz + 1] == np.float32(zero)), "entries equal to zero must not be emitted"
    return M.convert_sparse_vec_to_dense_vec(res, num_rows, zero)


# ------------------------------------------------------------------ SpMV plans of edge_matrix / wide_matrix with their structure asserted
PLAN_EXPORTS = ("entries", "bases", "units", "hub_rows", "hot", "hot_hdr", "present")
# (row blocks, column segments) through GRAPHLILY_DEBUG: the planner's own choice and a split plan.  The wide matrix keeps 16 row
# blocks in both (fewer entries per block = wider gaps between a block's sorted columns)
SPMV_SHAPES = {"edge": {"unsplit": (0, 0), "split": (5, 3)}, "wide": {"unsplit": (16, 1), "split": (16, 3)}}


def plan_formatters():
    from graphlily_amd import capi
    return (capi.GL_PLAN_HOST_FORMAT, capi.GL_PLAN_DEVICE_FORMAT)


def set_plan_knobs(monkeypatch, which, shape, hot=EDGE_HOT):
    """The planner overrides under which edge_matrix / wide_matrix reach their structures: a hot table of `hot` columns (0: none)
    and the (row blocks, column segments) of SPMV_SHAPES[which][shape]."""
    if which == "edge":
        set_knob(monkeypatch, "spmv_hot", hot)
        set_knob(monkeypatch, "spmv_hot_floor", 1)      # (the general layout asks 4 entries per row block of a hot column: few rows per block here)
    blocks, segments = SPMV_SHAPES[which][shape]
    set_knob(monkeypatch, "spmv_blocks", blocks)
    set_knob(monkeypatch, "spmv_segments", segments)


def spmv_plans(monkeypatch, which, layout, shape, m, flags=None, extra=0, hot=EDGE_HOT):
    """One plan per formatter flag, with the structure the cases rely on asserted and the formatters' arrays compared
    -> (plans, split)."""
    from graphlily_amd import capi
    if flags is None:
        flags = plan_formatters()
    set_plan_knobs(monkeypatch, which, shape, hot)
    plans = [capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, flags=f | extra) for f in flags]
    info = plans[0].info()
    assert info["layout"] == ("general" if layout == "general" else "pattern")
    assert (info["segments"] > 1) == (shape == "split")
    if which == "edge":
        assert info["hot_columns"] == hot and (info["hot_nnz"] > 0) == (hot > 0) and plans[0].export("hub_rows").size > 0
    else:
        assert info["groups"] * 64 > 1.3 * m.nnz          # the stream holds visibly more slots than entries: the dummies
    for p in plans[1:]:
        assert p.info()["finite_values"] == info["finite_values"]
        for name in PLAN_EXPORTS:
            assert np.array_equal(plans[0].export(name), p.export(name)), name
    return plans, info["segments"] > 1


# ------------------------------------------------------------------ the integer value types: an independent restatement, inputs
VAL_UNSIGNED, VAL_UFIXED = 1, 2          # GL_VAL_UNSIGNED, GL_VAL_UFIXED_32_8 (graphlily/global.h:62-64)
VALUE_TYPES = {"unsigned": VAL_UNSIGNED, "ufixed": VAL_UFIXED}
WORD_MAX = 0xffffffff
WORD_OPS = {"Arithmetic": 0, "Logical": 1, "Tropical": 2}


def word_one(vt):
    """a && b / a || b: 1 for `unsigned`, 1.0 = 1 << 24 for the fixed point."""
    return 1 << 24 if vt == VAL_UFIXED else 1


def word_zero(vt, op):
    """The semiring's own zero: 0, 0, UINT_INF / UFIXED_INF = 255.0 (global.h:78-79)."""
    if op != 2:
        return 0
    return WORD_MAX if vt == VAL_UNSIGNED else 255 << 24


def word_nonzero_zero(vt, op, ref=None):
    """A `zero` other than the semiring's: (+,x) a word that saturates (fixed point) or wraps (unsigned) most rows, (||,&&) 2 -- neither
    0 nor ONE --, (min,+) the median of `ref` (the result under the semiring's zero): about half of the rows come out as it."""
    if op == 0:
        return 250 << 24 if vt == VAL_UFIXED else 0xfffffff0
    if op == 1:
        return 2
    return int(np.sort(np.asarray(ref, np.uint32))[len(ref) // 2])


def _word_products(a, b, op, vt):
    """The (x) ALU on uint64 copies of the words (hw/ufixed_pe_fwd.h:27-45 and the assignment to ValT): unsigned wraps; the fixed
    point rounds a product half up to 24 fraction bits and clamps it, and clamps a sum."""
    a, b, top = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64), np.uint64(WORD_MAX)
    if op == 0:
        p = a * b                                                    # < 2^64
        return p & top if vt == VAL_UNSIGNED else np.minimum((p + np.uint64(1 << 23)) >> np.uint64(24), top)
    if op == 1:
        return np.where((a != 0) & (b != 0), np.uint64(word_one(vt)), np.uint64(0))
    s = a + b
    return s & top if vt == VAL_UNSIGNED else np.minimum(s, top)


def _word_rows(row_of, p, num_rows, op, vt, zero):
    """The (+) ALU folded over every row's products, the accumulator starting at `zero` (spmv_module.h:478-510).  The fixed point's
    clamped running sum of non-negative terms is min(exact sum, 2^32 - 1); a || b gives ONE as soon as one is applied, so a row
    without products keeps `zero` itself."""
    top = np.uint64(WORD_MAX)
    if op == 0:
        tot = np.zeros(num_rows, np.uint64)
        np.add.at(tot, row_of, p)                                    # < 2^64: fewer than 2^32 terms below 2^32
        tot += np.uint64(zero)
        return (tot & top if vt == VAL_UNSIGNED else np.minimum(tot, top)).astype(np.uint32)
    if op == 1:
        applied = np.bincount(row_of, minlength=num_rows) > 0
        hit = np.bincount(row_of, weights=(p != 0), minlength=num_rows) > 0
        return np.where(applied, np.where(hit | (zero != 0), word_one(vt), 0), zero).astype(np.uint32)
    out = np.full(num_rows, zero, np.uint64)
    np.minimum.at(out, row_of, p)
    return out.astype(np.uint32)


def words_expected(indptr, indices, data, x, op, vt, zero):
    """y = zero (+) A (x) x of the CSR in the value type vt, restated from the ALUs with numpy uint64 -- not the oracle."""
    ip = np.asarray(indptr).astype(np.int64)
    n, nnz = len(ip) - 1, int(ip[-1] - ip[0])
    row_of = np.repeat(np.arange(n), np.diff(ip))
    col = np.asarray(indices)[ip[0]:ip[0] + nnz].astype(np.int64)
    return _word_rows(row_of, _word_products(np.asarray(data)[ip[0]:ip[0] + nnz], np.asarray(x)[col], op, vt), n, op, vt, zero)


def words_expected_frontier(indptr, indices, data, v, num_rows, op, vt, zero):
    """The frontier form: the CSC's columns that the sparse vector v names, each as often as it is named, applied to a result that
    starts at `zero` (spmspv_module.h:445-497)."""
    cnt = int(v["index"][0])
    cols, xv = v["index"][1:cnt + 1].astype(np.int64), v["val"][1:cnt + 1]
    ip = np.asarray(indptr).astype(np.int64)
    lens = ip[cols + 1] - ip[cols]
    pos = np.repeat(ip[cols] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
    return _word_rows(np.asarray(indices)[pos].astype(np.int64), _word_products(np.asarray(data)[pos], np.repeat(xv, lens), op, vt),
                      num_rows, op, vt, zero)


def words_mask_spmv(y, mask, mask_type):
    """SpMV: the mask is compared with 0 and masked-off rows are the literal 0 (spmv_module.h:518-530)."""
    if mask_type == 0:
        return y
    on = (np.asarray(mask) == 0) if mask_type == 1 else (np.asarray(mask) != 0)
    return np.where(on, y, 0).astype(np.uint32)


def words_mask_spmspv(y, mask, mask_type, zero):
    """SpMSpV: the mask is compared with `zero` and masked-off rows are `zero` (spmspv_module.h:499-516)."""
    if mask_type == 0:
        return y
    on = (np.asarray(mask) == zero) if mask_type == 1 else (np.asarray(mask) != zero)
    return np.where(on, y, zero).astype(np.uint32)


def _draw_words(rng, k, hi):
    return rng.integers(0, hi, size=k, dtype=np.uint64).astype(np.uint32)


def _sprinkle(rng, w, top=True, near_max=False):
    """The words every type has corners at: 5 % zeros (dropped by &&), 2 % 0x80000000 (a float -0.0, negative as an int), and for
    (min,+) 3 % 0xfffffff0 (saturates in the fixed point, wraps in unsigned when something is added)."""
    u = rng.random(w.shape[0])
    w[u < 0.05] = 0
    if top:
        w[(u >= 0.05) & (u < 0.07)] = 0x80000000
    if near_max:
        w[(u >= 0.07) & (u < 0.10)] = 0xfffffff0
    return w


def _word_ranges(vt, op, kind):
    """(matrix words below, x words below).  (+,x) `small`: products below 2^15 -- no row of edge_matrix saturates, the hub rows'
    sums come out exactly; `large`: products up to 2^31 = 128.0 -- rows of more than about 8 entries saturate.  The other semirings:
    `frontier` (SpMSpV): products up to 2^30, a row saturates
    from about 16 columns on.  The other semirings: the fixed point below 8.0 / 120.0, unsigned below 2^20 / 2^28."""
    if op == 0:
        return {"small": (1 << 25, 1 << 14), "large": (1 << 25, 1 << 30), "frontier": (1 << 25, 1 << 29)}[kind]
    return (8 << 24, 120 << 24) if vt == VAL_UFIXED else (1 << 20, 1 << 28)


HUB_SMALL_ROW, HUB_CROSSING_ROW, HUB_CROSSING_WORD = 7, 1000, 98304


def typed_inputs(rng, m, layout, vt, op, kind=None):
    """(data words, x words, mask words, zero word) for the CSR m in the value type vt and the semiring op.  Layout `general`: a word
    per entry; `pattern`: per column; `pattern_diag`: so, with a diagonal word that differs from its column's.  Masks are drawn from
    {0, 1, 0x80000000}; the corner words of _sprinkle are in the matrix and in x ((+,x) `small` keeps 0x80000000 out of x: times a
    matrix word it saturates on its own).  (||,&&) and (min,+): x is the semiring's zero on half of the columns.  (+,x) `large` on the general
    layout of edge_matrix: hub row 7 gets words below 2^12 (it stays unsaturated) and hub row 1000 the constant word 98304, with which
    its sum is about 1.5 x 2^32 while any column-contiguous half of its entries stays below 2^32."""
    nnz, nc = m.nnz, m.num_cols
    ip = m.adj_indptr.astype(np.int64)
    col = m.adj_indices[:nnz].astype(np.int64)
    row = np.repeat(np.arange(m.num_rows), np.diff(ip))
    a_hi, x_hi = _word_ranges(vt, op, kind)
    zero = word_zero(vt, op)
    a = _sprinkle(rng, _draw_words(rng, nnz if layout == "general" else nc, a_hi), near_max=op == 2)
    x = _sprinkle(rng, _draw_words(rng, nc, x_hi), top=not (op == 0 and kind == "small"), near_max=op == 2)
    if op != 0:
        x[rng.random(nc) < 0.5] = zero
    if layout != "general":
        a = a[col]
        if layout == "pattern_diag":
            d = np.flatnonzero(col == row)
            alt = _sprinkle(rng, _draw_words(rng, len(d), a_hi), near_max=op == 2)
            a[d] = np.where(alt == a[d], alt ^ np.uint32(1), alt)
    elif op == 0 and kind == "large" and m.num_rows > HUB_CROSSING_ROW:
        lo, hi = ip[HUB_SMALL_ROW], ip[HUB_SMALL_ROW + 1]
        a[lo:hi] = _draw_words(rng, hi - lo, 1 << 12)
        a[ip[HUB_CROSSING_ROW]:ip[HUB_CROSSING_ROW + 1]] = HUB_CROSSING_WORD
    mask = rng.choice(np.array([0, 1, 0x80000000], np.uint32), size=m.num_rows)
    return np.ascontiguousarray(a, np.uint32), x, mask, zero


def word_vec(indices, vals):
    """A sparse vector of value words: [0] = {count, -}, the entries behind it."""
    v = np.zeros(len(indices) + 1, dtype=O.IDX_WORD)
    v["index"][0] = len(indices)
    v["index"][1:] = indices
    v["val"][1:] = vals
    return v


def frontier_words(rng, vt, op, k, kind=None):
    """k x words for a frontier (typed_inputs' ranges and corner words; (min,+): none equal to the semiring's zero)."""
    return _sprinkle(rng, _draw_words(rng, k, _word_ranges(vt, op, kind)[1]), top=not (op == 0 and kind == "small"), near_max=op == 2)


def csc_words(rng, nnz, vt, op, kind=None):
    """A word per stored entry of a CSC (typed_inputs' ranges and corner words)."""
    return _sprinkle(rng, _draw_words(rng, nnz, _word_ranges(vt, op, kind)[0]), near_max=op == 2)


def spmspv_mask_words(rng, num_rows, zero):
    """SpMSpV compares its mask with `zero`: a third of the rows hold it, a third 7 and a third 0x80000000 (equal to 0 as a float)."""
    return rng.choice(np.array([zero, 7, 0x80000000], np.uint32), size=num_rows)


def _csc_from_keys(n, key):
    """CSC structure (values 1) of the distinct keys column * n + row."""
    key = np.unique(np.asarray(key, np.int64))
    indptr = np.zeros(n + 1, np.uint32)
    np.cumsum(np.bincount(key // n, minlength=n), out=indptr[1:])
    return io.CSCMatrix(n, n, np.ones(key.shape[0], np.float32), (key % n).astype(np.uint32), indptr)


def long_columns_csc():
    """16384 x 16384 with 24 columns of 4097 .. 8191 entries (four of 4097: just above the 4096-entry chunk) and nothing else: with all
    of them in the frontier the columns are shared between workgroups by chunks, and with every column named twice the bins
    overflow into the dense accumulator -> (csc, the 24 columns)."""
    rng = np.random.default_rng(17)
    n = 16384
    degs = rng.integers(4097, 8192, size=24)
    degs[:4] = 4097
    cols = np.sort(rng.choice(n, size=24, replace=False))
    key = np.concatenate([c * n + rng.choice(n, size=int(d), replace=False) for c, d in zip(cols, degs)])
    return _csc_from_keys(n, key), cols.astype(np.uint32)


def random_csc(n, avg, seed, hub=None):
    """n x n, 0 .. 2 avg distinct random rows per column; hub = (count, length): that many columns of that length."""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(n), rng.integers(0, 2 * avg + 1, size=n))
    keys = [col * n + rng.integers(0, n, size=col.shape[0])]
    if hub:
        keys += [c * n + rng.choice(n, size=hub[1], replace=False) for c in rng.choice(n, size=hub[0], replace=False)]
    return _csc_from_keys(n, np.concatenate(keys))


CONTENDED_N = 131136                 # 2049 row tiles of 64: one more than the SpMSpV bin kernel has counters for
CONTENDED_ROWS = (0, 1)


def contended_csc(n=CONTENDED_N):
    """n x n with 6 random rows (from row 2 on) per column and the rows 0 and 1 in every 4th column: whatever the frontier, a
    quarter of its columns meet in these two rows."""
    rng = np.random.default_rng(n)
    c = np.repeat(np.arange(n), 6)
    c4 = np.arange(0, n, 4)
    return _csc_from_keys(n, np.concatenate([c * n + rng.integers(2, n, size=c.shape[0]), c4 * n, c4 * n + 1]))


def contended_words(rng, csc, vt, op):
    """csc_words for contended_csc; for (+,x), whose x words are below 2^29 (`frontier`), row 0 holds 1.0 -- in the fixed point it
    saturates from about 16 columns on -- and row 1 holds 2^-14: a few thousand columns leave it far below 2^32."""
    a = csc_words(rng, csc.nnz, vt, op, "frontier")
    if op == 0:
        a[csc.adj_indices == 0] = 1 << 24
        a[csc.adj_indices == 1] = 1 << 10
    return a


# ---- the SpMSpV cases of the integer value types, shared by tests/test_typed_edges_cpu.py (which proves them on the oracle) and
# tests/test_gpu_typed_edges.py.  The structures are built once and shared: callers do not write to them.
long_columns_csc = functools.lru_cache(maxsize=None)(long_columns_csc)
contended_csc = functools.lru_cache(maxsize=None)(contended_csc)
random_csc = functools.lru_cache(maxsize=None)(random_csc)


@functools.lru_cache(maxsize=None)
def rmat_sssp_csc():
    """rmat_20K with SSSP's self edges, padded to a multiple of 128, by columns: no column longer than 12288 entries, so a
    mid-size vector is cut by entries unless the knob forces the cut by products."""
    m = named_matrix("rmat_20K")
    io.sssp_add_self_edges(m)
    io.util_round_csr_matrix_dim(m, 128, 128)
    return io.csr2csc(m)


@functools.lru_cache(maxsize=None)
def rmat_csc():
    return io.csr2csc(named_matrix("rmat_20K"))


def spmspv_kind(op):
    return "frontier" if op == 0 else None


def long_columns_case(vt_name, op):
    """The long-column matrix in words -> (csc, data, [v, v doubled, v], mask, zero): the doubled vector names every column twice,
    with a second set of x words."""
    vt = VALUE_TYPES[vt_name]
    csc, cols = long_columns_csc()
    rng = np.random.default_rng(stable_seed("long columns", vt_name, op))
    zero = word_zero(vt, op)
    data = csc_words(rng, csc.nnz, vt, op, spmspv_kind(op))
    xv, xv2 = (frontier_words(rng, vt, op, len(cols), spmspv_kind(op)) for _ in range(2))
    v, v2 = word_vec(cols, xv), word_vec(np.concatenate([cols, cols]), np.concatenate([xv, xv2]))
    return csc, data, [v, v2, v], spmspv_mask_words(rng, csc.num_rows, zero), zero


def contended_case(vt_name, op):
    """contended_csc in words with frontiers of 300 and 5000 columns -> (csc, data, [v300, v5000], mask, zero)."""
    vt = VALUE_TYPES[vt_name]
    csc = contended_csc()
    rng = np.random.default_rng(stable_seed("contended", vt_name, op))
    zero = word_zero(vt, op)
    data = contended_words(rng, csc, vt, op)
    vs = []
    for cnt in (300, 5000):
        cols = np.sort(rng.choice(csc.num_cols, size=cnt, replace=False)).astype(np.uint32)
        vs.append(word_vec(cols, frontier_words(rng, vt, op, cnt, spmspv_kind(op))))
    return csc, data, vs, spmspv_mask_words(rng, csc.num_rows, zero), zero


def frontier_case(csc, name, vt_name, op, counts):
    """Any CSC structure in words with frontiers of `counts` random columns -> (data, [v ...], mask, zero)."""
    vt = VALUE_TYPES[vt_name]
    rng = np.random.default_rng(stable_seed(name, vt_name, op))
    zero = word_zero(vt, op)
    data = csc_words(rng, csc.nnz, vt, op, spmspv_kind(op))
    vs = []
    for cnt in counts:
        cols = np.sort(rng.choice(csc.num_cols, size=cnt, replace=False)).astype(np.uint32)
        vs.append(word_vec(cols, frontier_words(rng, vt, op, cnt, spmspv_kind(op))))
    return data, vs, spmspv_mask_words(rng, csc.num_rows, zero), zero


def spmv_words_reference(m, a, x, op, vt, zero, mask=None, mask_type=0):
    """What a typed SpMV run must give, word for word: the oracle's O.spmv_words -- with one documented difference.  The library
    computes y = zero (+) sum (graphlily_hip.h), so under (||,&&) a row WITHOUT stored entries gives zero || nothing = ONE when
    `zero` is non-zero, where the reference's loop never applies || to such a row and leaves `zero` itself; the two agree on every
    other row and for every zero a driver uses (0).  tests/test_typed_edges_cpu.py proves that these rows are the only difference."""
    ref = O.spmv_words(m.adj_indptr, m.adj_indices, a, x, op, vt, zero, mask if mask_type else None, mask_type)
    if op == 1 and zero != 0:
        empty = np.diff(m.adj_indptr.astype(np.int64)) == 0
        ref = np.where(empty, words_mask_spmv(np.full(m.num_rows, word_one(vt), np.uint32), mask, mask_type), ref).astype(np.uint32)
    return ref
