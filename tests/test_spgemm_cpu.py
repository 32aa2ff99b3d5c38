"""The host side of SpGEMM (gl_spgemm_symbolic / gl_spgemm_numeric, app.validate_spgemm): spgemm_model -- the definition of
include/graphlily_hip_spgemm.h as a loop over the non-empty rows, the truth tests/test_gpu_spgemm.py compares the kernels with --
against a dense numpy product, validate_spgemm on the model's C and on four ways of spoiling it, and the extension's header
against its own capi.EXT_HEADERS entry and the library."""
import math
import os
import re

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver
from test_tc_cpu import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPGEMM_DRIVER = os.path.join(ROOT, "build", "spgemm_driver")
GOLDEN = "spgemm_directed_csr_float32.npz"
HEADER = "graphlily_hip_spgemm.h"
SEMIRINGS = {"muladd": M.kMulAdd, "andor": M.kLogicalAndOr, "addmin": M.kAddMin}
MASKS = {"none": (False, False), "mask": (True, False), "complement": (True, True)}


def spgemm_model(a, b, op, mask=None, complement=False):
    """-> (C as io.CSRMatrix, columns ascending; products per entry as int64[nnz]).  (+,x): the f32 nearest the math.fsum of the
    exact f64 products; (min,+): the minimum of the f32 sums; (||,&&): 1."""
    n = a.num_rows
    ap, bp = a.adj_indptr.astype(np.int64), b.adj_indptr.astype(np.int64)
    mp = mask.adj_indptr.astype(np.int64) if mask is not None else None
    indptr, cols, vals, counts = np.zeros(n + 1, np.int64), [], [], []
    for i in np.flatnonzero(np.diff(ap)).tolist():
        terms = {}
        for e in range(ap[i], ap[i + 1]):
            k = int(a.adj_indices[e])
            for f in range(bp[k], bp[k + 1]):
                terms.setdefault(int(b.adj_indices[f]), []).append((a.adj_data[e], b.adj_data[f]))
        if mask is not None:
            stored = set(mask.adj_indices[mp[i]:mp[i + 1]].tolist())
            terms = {j: t for j, t in terms.items() if (j in stored) != complement}
        for j in sorted(terms):
            t = terms[j]
            cols.append(j)
            counts.append(len(t))
            vals.append(1.0 if op == M.kLogicalAndOr else min(x + y for x, y in t) if op == M.kAddMin
                        else np.float32(math.fsum(float(x) * float(y) for x, y in t)))
        indptr[i + 1] = len(terms)
    return io.CSRMatrix(n, n, np.array(vals, np.float32), np.array(cols, np.uint32), np.cumsum(indptr)), np.array(counts, np.int64)


def random_csr(n, m, seed, values="int"):
    """m distinct entries of an n x n matrix; values: small positive integers, or signed reals"""
    rng = np.random.default_rng(seed)
    key = rng.choice(n * n, size=m, replace=False)
    data = rng.integers(1, 4, m) if values == "int" else rng.standard_normal(m)
    return _csr(n, key // n, key % n, data.astype(np.float32))


def dense(m):
    """-> (f64 values, stored?)"""
    v, s = np.zeros((m.num_rows, m.num_cols)), np.zeros((m.num_rows, m.num_cols), bool)
    rows = np.repeat(np.arange(m.num_rows), np.diff(m.adj_indptr.astype(np.int64)))
    v[rows, m.adj_indices] = m.adj_data
    s[rows, m.adj_indices] = True
    return v, s


@pytest.mark.parametrize("values", ["int", "real"])
@pytest.mark.parametrize("masking", sorted(MASKS))
@pytest.mark.parametrize("semiring", sorted(SEMIRINGS))
def test_model_equals_the_dense_product_and_validates(semiring, masking, values):
    n, op = 61, SEMIRINGS[semiring]
    a, b, mask = random_csr(n, 400, 1, values), random_csr(n, 380, 2, values), random_csr(n, 900, 3)
    use_mask, complement = MASKS[masking]
    c, counts = spgemm_model(a, b, op, mask if use_mask else None, complement)
    (av, as_), (bv, bs), (_, ms) = dense(a), dense(b), dense(mask)
    pattern = (as_.astype(np.int64) @ bs.astype(np.int64)) > 0
    if use_mask:
        pattern &= ms != complement
    got_v, got_s = dense(c)
    assert np.array_equal(got_s, pattern) and int(counts.sum()) == int((as_.astype(np.int64) @ bs.astype(np.int64))[pattern].sum())
    for i, j in zip(*np.nonzero(pattern)):
        k = np.flatnonzero(as_[i] & bs[:, j])
        if op == M.kLogicalAndOr:
            want = 1.0
        elif op == M.kAddMin:
            want = float(np.min(av[i, k].astype(np.float32) + bv[k, j].astype(np.float32)))
        elif values == "int":
            want = float(av[i].astype(np.int64) @ bv[:, j].astype(np.int64))
        else:
            want = float(np.float32(math.fsum((av[i, k] * bv[k, j]).tolist())))
        assert got_v[i, j] == want, (i, j)
    assert app.validate_spgemm(a, b, c, op, mask if use_mask else None, complement) == c.nnz


def _spoiled(c, how):
    ip = c.adj_indptr.astype(np.int64)
    row = int(np.argmax(np.diff(ip)))                       # a row of several entries
    at = int(ip[row])
    idx, val, ptr = c.adj_indices.copy(), c.adj_data.copy(), ip.copy()
    if how == "missing":
        idx, val = np.delete(idx, at), np.delete(val, at)
        ptr[row + 1:] -= 1
    elif how == "extra":
        free = int(np.setdiff1d(np.arange(c.num_cols), idx[ip[row]:ip[row + 1]])[-1])
        at = int(ip[row + 1])
        idx, val = np.insert(idx, at, free), np.insert(val, at, 1.0)
        ptr[row + 1:] += 1
    elif how == "swapped":
        idx[[at, at + 1]], val[[at, at + 1]] = idx[[at + 1, at]], val[[at + 1, at]]
    else:
        val[at] = np.nextafter(np.nextafter(val[at], np.float32(np.inf)), np.float32(np.inf))
    return io.CSRMatrix(c.num_rows, c.num_cols, val, idx, ptr)


@pytest.mark.parametrize("how,message", [("missing", "missing columns"), ("extra", "do not belong"), ("swapped", "do not ascend"),
                                         ("two_ulps", "products give")])
def test_validate_rejects(how, message):
    a = random_csr(61, 400, 1, "real")
    c, _ = spgemm_model(a, a, M.kMulAdd)
    with pytest.raises(ValueError, match=message):
        app.validate_spgemm(a, None, _spoiled(c, how), M.ArithmeticSemiring)


def test_library_exports_and_binds_the_entry_points():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    names = ["gl_spgemm_numeric", "gl_spgemm_symbolic"]
    assert all(hasattr(L, f) for f in names), "libgraphlily_hip.so does not export gl_spgemm_*"
    assert len(L.gl_spgemm_symbolic.argtypes) == 6 and len(L.gl_spgemm_numeric.argtypes) == 11
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert '#include "graphlily_hip.h"' in text and 'extern "C"' in text and "#define GL_SPGEMM_MASK_COMPLEMENT 1u" in text
    assert sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))) == capi.EXT_HEADERS[HEADER] == names
    assert not set(names) & (set(capi.EXPORTS) | set(capi.EXT_EXPORTS))
    assert callable(capi.SpMVPlan.spgemm_symbolic) and callable(capi.SpMVPlan.spgemm_numeric)
    assert callable(M.SpGEMMModule.run) and callable(app.TwoHop.run) and callable(app.validate_spgemm)
    if capi.device_count() == 0:
        assert L.gl_spgemm_symbolic(None, None, None, 0, None, None) == capi.GL_ERR_NOT_INITIALIZED


def test_cpp_driver_compiles_without_warnings():
    assert build_cpp_driver("spgemm_driver.cpp") == SPGEMM_DRIVER

