"""CPU tests of the manual averaging's boundary (include/fdoct_manualavg.h) on the built library, without a device: the exports,
the function-try-block at every entry point, fdoct_manualavg_plan against the model, and error codes instead of crashes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
import manualavg_model as m
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def test_manualavg_header_is_exported_and_listed_and_on_its_own():
    declared = _declared("fdoct_manualavg.h")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", fdoct_amd.library_path()], text=True)
    exported = sorted(s for s in re.findall(r"\bT (fdoct_\w+)$", nm, re.M) if s.startswith("fdoct_manualavg"))
    assert declared == exported == sorted(capi.MANUALAVG_ABI_SYMBOLS) and len(declared) == 5
    assert all(s.startswith("fdoct_manualavg_") for s in declared)
    assert not [s for s in declared if s.startswith("fdoct_bscan") or "colour" in s]   # the binning's and the colour header's claims
    others = [capi.ABI_SYMBOLS, capi.ROI_ABI_SYMBOLS, capi.CAPTURE_ABI_SYMBOLS, capi.LOWPASS_ABI_SYMBOLS, capi.BSCANBIN_ABI_SYMBOLS,
              capi.COLOUR_ABI_SYMBOLS]
    for other in others:
        assert not set(declared) & set(other)
    base = open(os.path.join(ROOT, "include", "fdoct.h")).read()
    assert "manualav" not in base and "manualaccum" not in base
    assert sorted(capi.ABI_SYMBOLS) == _declared("fdoct.h") and len(capi.ABI_SYMBOLS) == 50
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)


def test_every_manualavg_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_manualavg.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.MANUALAVG_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"
    base = [d[0] for d in _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_capi.cpp"))]
    assert len(base) == 50 and not set(base) & set(names)


def test_manualavg_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_manualavg.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_manualavg.h"
int main(void) {
  int (*plan)(int, int, int, int, int*, int*) = fdoct_manualavg_plan;
  int (*begin)(fdoct_handle, int, size_t, int) = fdoct_manualavg_begin;
  int (*add)(fdoct_handle, const float*, fdoct_memspace, int, float*, float*, fdoct_memspace, int, int*) = fdoct_manualavg_add;
  int (*state)(fdoct_handle, int*, size_t*, int*, int*, double*) = fdoct_manualavg_state;
  int (*end)(fdoct_handle) = fdoct_manualavg_end;
  fdoct_manualavg_mode mode = FDOCT_MANUALAVG_KEEP_ALL;
  (void)plan; (void)begin; (void)add; (void)state; (void)end;
  return mode == 1 && FDOCT_MANUALAVG_REFERENCE == 0 ? 0 : 1;
}
""")
    obj = tmp_path / "use_manualavg.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    assert obj.exists()


def test_plan_agrees_with_the_model():
    for mode in (m.REFERENCE, m.KEEP_ALL):
        for avg in range(1, 6):
            for accumulated in range(avg + 1):
                for n in range(14):
                    assert capi.manualavg_plan(avg, mode, accumulated, n) == m.plan(avg, mode, accumulated, n), (mode, avg, accumulated, n)
    assert capi.manualavg_plan(2, capi.MANUALAVG_REFERENCE, 0, 7) == (2, 1)
    assert capi.manualavg_plan(2, capi.MANUALAVG_KEEP_ALL, 0, 7) == (3, 1)
    assert capi.manualavg_plan(7, capi.MANUALAVG_REFERENCE, 0, 64) == (8, 0)
    assert capi.manualavg_plan(1, capi.MANUALAVG_REFERENCE, 1, 2 ** 31 - 1) == (2 ** 30, 0)
    assert (capi.MANUALAVG_REFERENCE, capi.MANUALAVG_KEEP_ALL) == (m.REFERENCE, m.KEEP_ALL)


def test_plan_refuses_bad_arguments_and_its_outputs_are_optional():
    for bad in [(0, 0, 0, 1), (-3, 0, 0, 1), (2, 2, 0, 1), (2, -1, 0, 1), (2, 0, 3, 1), (2, 1, 3, 1), (2, 0, -1, 1), (2, 0, 0, -1)]:
        with pytest.raises(fdoct_amd.FdoctError) as e:
            capi.manualavg_plan(*bad)
        assert e.value.code == INVALID
    lib = fdoct_amd.load_library()
    assert b"fdoct_manualavg_plan" in lib.fdoct_last_error(None)
    e, a = C.c_int(-7), C.c_int(-7)
    assert lib.fdoct_manualavg_plan(3, 0, 1, 9, None, None) == 0
    assert lib.fdoct_manualavg_plan(3, 0, 1, 9, C.byref(e), None) == 0 and lib.fdoct_manualavg_plan(3, 0, 1, 9, None, C.byref(a)) == 0
    assert (e.value, a.value) == m.plan(3, 0, 1, 9)
    e.value = -7
    assert lib.fdoct_manualavg_plan(0, 0, 0, 1, C.byref(e), None) == INVALID and e.value == -7


def test_a_null_handle_is_invalid_everywhere():
    lib = fdoct_amd.load_library()
    buf = np.zeros(3 * 16, np.float32)
    src, mean, db = buf[:16].ctypes.data, buf[16:32].ctypes.data, buf[32:].ctypes.data
    n = C.c_int(-7)
    assert lib.fdoct_manualavg_begin(None, 2, 16, 0) == INVALID
    assert lib.fdoct_manualavg_begin(None, 0, 16, 0) == INVALID and lib.fdoct_manualavg_begin(None, 2, 0, 0) == INVALID
    assert lib.fdoct_manualavg_begin(None, 2, 16, 2) == INVALID
    assert lib.fdoct_manualavg_add(None, src, 0, 1, mean, db, 0, 1, C.byref(n)) == INVALID and n.value == -7
    assert lib.fdoct_manualavg_add(None, None, 0, 1, mean, db, 0, 1, None) == INVALID
    assert lib.fdoct_manualavg_add(None, src, 2, 1, mean, db, 0, 1, None) == INVALID
    assert lib.fdoct_manualavg_add(None, src, 0, 0, mean, db, 0, 1, None) == INVALID
    assert lib.fdoct_manualavg_state(None, None, None, None, C.byref(n), None) == INVALID and n.value == -7
    assert lib.fdoct_manualavg_end(None) == INVALID
    assert not buf.any()
