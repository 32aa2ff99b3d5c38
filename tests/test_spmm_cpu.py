"""The host side of SpMM (gl_spmm, app.validate_spmm): the validator on a hand-written 4 x 3 case under each semiring and on two
ways of spoiling it, the extension's header against its own capi.EXT_HEADERS entry and the library, and the C++ driver's build."""
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPMM_DRIVER = os.path.join(ROOT, "build", "spmm_driver")
HEADER = "graphlily_hip_spmm.h"

# A = [[2, 0, -1], [0, 0, 0], [0.5, 0.5, 0], [0, 4, 4]] with (3, 1) and (3, 2) stored; row 1 is empty
A = io.CSRMatrix(4, 3, [2, -1, 0.5, 0.5, 4, 4], [0, 2, 0, 1, 1, 2], [0, 2, 2, 4, 6])
X = np.array([[1, 0], [3, 0], [-2, 5]], np.float32)
MASK = np.array([[1, 0], [0, 1], [1, 1], [0, 0]], np.float32)
INF = M.TropicalSemiring.zero
EXPECTED = {
    "muladd": (M.ArithmeticSemiring, [[4, -5], [0, 0], [2, 0], [4, 20]]),
    "andor": (M.LogicalSemiring, [[1, 1], [0, 0], [1, 0], [1, 1]]),
    "addmin": (M.TropicalSemiring, [[-3, 2], [INF, INF], [1.5, 0.5], [2, 4]]),
}


@pytest.mark.parametrize("semiring", sorted(EXPECTED))
def test_validate_accepts_the_hand_written_case_and_rejects_it_spoiled(semiring):
    s, y = EXPECTED[semiring][0], np.array(EXPECTED[semiring][1], np.float32)
    assert app.validate_spmm(A, X, y, s) == 8
    assert app.validate_spmm(A, X, np.where(MASK != 0, y, 0), s, MASK, M.kMaskWriteToOne) == 8
    assert app.validate_spmm(A, X, np.where(MASK == 0, y, 0), s, MASK, M.kMaskWriteToZero, rows=(1, 3)) == 4
    off = y.copy()
    off[3, 1] = np.nextafter(np.nextafter(off[3, 1], np.float32(np.inf)), np.float32(np.inf))       # two ulps: above the bound
    with pytest.raises(ValueError, match=r"Y\[3, 1\] is .* entries of the row give"):
        app.validate_spmm(A, X, off, s)
    masked = np.where(MASK != 0, y, 0)
    masked[0, 1] = 1e-30
    with pytest.raises(ValueError, match=r"Y\[0, 1\] .* must be the literal 0"):
        app.validate_spmm(A, X, masked, s, MASK, M.kMaskWriteToOne)


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_spmm"), "libgraphlily_hip.so does not export gl_spmm"
    assert len(L.gl_spmm.argtypes) == 13
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert '#include "graphlily_hip.h"' in text and 'extern "C"' in text and "0xffffffff" in raw
    assert sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))) == capi.EXT_HEADERS[HEADER] == ["gl_spmm"]
    assert "gl_spmm" not in capi.EXPORTS and "gl_spmm" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.spmm) and callable(M.SpMMModule.run) and callable(app.validate_spmm)
    if capi.device_count() == 0:
        assert L.gl_spmm(None, None, None, 0, None, 0, None, 0, 0, 0, 0.0, 0, None) == capi.GL_ERR_NOT_INITIALIZED


def test_cpp_driver_compiles_and_fails_loudly_without_gpu():
    assert build_cpp_driver("spmm_driver.cpp") == SPMM_DRIVER
    if capi.device_count() == 0:
        r = subprocess.run([SPMM_DRIVER], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
