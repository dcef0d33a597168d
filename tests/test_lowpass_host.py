"""CPU tests of the boundary of include/fdoct_lowpass.h (BscanDark's lpfilter and the capture's options): the exports, the
function-try-block at every entry point, the header as C99, and error codes instead of crashes without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fdoct_amd
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fdoct_get_capture_options", "fdoct_lowpass_rows", "fdoct_set_capture_options"]


def test_lowpass_header_is_exported_and_listed_and_disjoint_from_the_other_headers():
    declared = _declared("fdoct_lowpass.h")
    assert declared == NAMES
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(capi.LOWPASS_ABI_SYMBOLS) == declared
    for other in (capi.ABI_SYMBOLS, capi.ROI_ABI_SYMBOLS, capi.CAPTURE_ABI_SYMBOLS):
        assert not set(declared) & set(other)
    # the other headers name what they named before
    assert sorted(capi.CAPTURE_ABI_SYMBOLS) == _declared("fdoct_capture.h")
    assert sorted(capi.ROI_ABI_SYMBOLS) == _declared("fdoct_roi.h")
    assert sorted(capi.ABI_SYMBOLS) == _declared("fdoct.h")


def test_every_lowpass_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_lowpass.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and sorted(names) == NAMES
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_lowpass_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_lowpass.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_capture.h"
#include "fdoct_lowpass.h"
int main(void) {
  int (*set)(fdoct_handle, int, int) = fdoct_set_capture_options;
  int (*get)(fdoct_handle, int*, int*) = fdoct_get_capture_options;
  int (*lp)(fdoct_handle, const double*, fdoct_memspace, int, int, size_t, double*, fdoct_memspace) = fdoct_lowpass_rows;
  (void)set; (void)get; (void)lp;
  return 0;
}
""")
    obj = tmp_path / "use_lowpass.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    assert obj.exists()


def test_lowpass_entry_points_refuse_a_null_handle_without_a_device():
    lib = fdoct_amd.load_library()
    x = np.zeros(64, np.float64)
    a, b = C.c_int(7), C.c_int(7)
    assert lib.fdoct_set_capture_options(None, 1, 1) == -1
    assert lib.fdoct_get_capture_options(None, C.byref(a), C.byref(b)) == -1 and (a.value, b.value) == (7, 7)
    assert lib.fdoct_lowpass_rows(None, x.ctypes.data, capi.MEM_HOST, 1, 64, 0, x.ctypes.data, capi.MEM_HOST) == -1
    assert lib.fdoct_lowpass_rows(None, None, capi.MEM_HOST, 0, 0, 1, None, 5) == -1     # bad arguments and no handle
    assert np.all(x == 0.0)
    for name in ("set_capture_options", "get_capture_options", "lowpass_rows", "lowpass_rows_device"):
        assert callable(getattr(fdoct_amd.Reconstructor, name))
