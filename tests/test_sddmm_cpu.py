"""The host side of SDDMM (gl_sddmm, app.validate_sddmm): the validator on a hand-written 4 x 3 pattern with k = 2 under each
semiring and on two ways of spoiling it, the extension's header against its own capi.EXT_HEADERS entry and the library, and the
C++ driver's build."""
import os
import re
import subprocess

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M

from helpers import build_cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDDMM_DRIVER = os.path.join(ROOT, "build", "sddmm_driver")
HEADER = "graphlily_hip_sddmm.h"

# the entries (0, 0), (0, 2), (2, 0), (2, 1), (3, 1) and a marker in row 3; row 1 is empty
A = io.CSRMatrix(4, 3, [2, -1, 0.5, 0.5, 4, 9], [0, 2, 0, 1, 1, 0xffffffff], [0, 2, 2, 4, 6])
X = np.array([[1, 0], [7, 7], [3, 0], [-2, 5]], np.float32)
Y = np.array([[1, 2], [0, 4], [-1, 0.5]], np.float32)
EXPECTED = {        # semiring -> (scaled by A's values, the bracket itself)
    "muladd": (M.ArithmeticSemiring, [2, 1, 1.5, 0, 80, 0], [1, -1, 3, 0, 20, 0]),
    "andor": (M.LogicalSemiring, [1, 1, 1, 0, 1, 0], [1, 1, 1, 0, 1, 0]),
    "addmin": (M.TropicalSemiring, [4, -1, 2.5, 3.5, 2, 0], [2, 0, 2, 3, -2, 0]),
}


@pytest.mark.parametrize("semiring", sorted(EXPECTED))
def test_validate_accepts_the_hand_written_case_and_rejects_it_spoiled(semiring):
    s, scaled, plain = EXPECTED[semiring]
    scaled, plain = np.array(scaled, np.float32), np.array(plain, np.float32)
    assert app.validate_sddmm(A, X, Y, scaled, s) == 6
    assert app.validate_sddmm(A, X, Y, plain, s, scaled=False) == 6
    assert app.validate_sddmm(A, X, Y, scaled[2:], s, rows=(2, 4)) == 4
    off = scaled.copy()
    off[4] = np.nextafter(np.nextafter(off[4], np.float32(np.inf)), np.float32(np.inf))       # two ulps: above the bound
    with pytest.raises(ValueError, match=r"out\[4\] = C\[3, 1\] is .* features give"):
        app.validate_sddmm(A, X, Y, off, s)
    marked = scaled.copy()
    marked[5] = 1e-30
    with pytest.raises(ValueError, match=r"out\[5\] .* must be the literal 0"):
        app.validate_sddmm(A, X, Y, marked, s)


def test_library_exports_and_binds_the_entry_point():
    """this extension's own header against its own entry of capi.EXT_HEADERS and the library; nothing about other entries"""
    L = capi.lib()
    assert hasattr(L, "gl_sddmm"), "libgraphlily_hip.so does not export gl_sddmm"
    assert len(L.gl_sddmm.argtypes) == 11
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert '#include "graphlily_hip.h"' in text and 'extern "C"' in text and "0xffffffff" in raw
    assert sorted(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))) == capi.EXT_HEADERS[HEADER] == ["gl_sddmm"]
    assert "gl_sddmm" not in capi.EXPORTS and "gl_sddmm" not in capi.EXT_EXPORTS
    assert callable(capi.SpMVPlan.sddmm) and callable(M.SDDMMModule.run) and callable(app.validate_sddmm)
    if capi.device_count() == 0:
        assert L.gl_sddmm(None, None, None, 0, None, 0, None, 0, 0, 0.0, None) == capi.GL_ERR_NOT_INITIALIZED


def test_cpp_driver_compiles_and_fails_loudly_without_gpu():
    assert build_cpp_driver("sddmm_driver.cpp") == SDDMM_DRIVER
    if capi.device_count() == 0:
        r = subprocess.run([SDDMM_DRIVER], capture_output=True, text=True)
        assert r.returncode != 0
        assert "gl_init" in r.stdout + r.stderr       # print-and-exit convention of the reference
